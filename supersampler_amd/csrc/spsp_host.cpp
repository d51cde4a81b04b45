// spsp_host.cpp -- the host side of the two CLIs behind the C-ABI: FASTA
// ingest, sketch (de)serialisation, CSV printing and zstr-compatible file I/O.
// These are the stages SURVEY.md 8(a) keeps on the host (A4, A7-A11, A16);
// they work on 2-bit integers throughout instead of the reference's
// std::string substr/find chains, but produce the same bytes.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "spsp_internal.h"

typedef unsigned __int128 u128;

namespace {

using spsp::set_error;
using spsp::now_s;

inline uint32_t code_of(uint8_t c) { return (c >> 1) & 3u; }  // A=0 C=1 T=2 G=3 (utils.cpp:13-16)
const char kNuc[4] = {'A', 'C', 'T', 'G'};                     // int2nuc (utils.cpp:26-45)

template <class T> T* dup_vec(const std::vector<T>& v) {
    T* p = (T*)malloc(std::max<size_t>(1, v.size()) * sizeof(T));
    if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

inline uint64_t rev_groups64(uint64_t x) {  // reverse the 32 two-bit groups
    x = __builtin_bswap64(x);
    x = ((x & 0x0f0f0f0f0f0f0f0fULL) << 4) | ((x >> 4) & 0x0f0f0f0f0f0f0f0fULL);
    x = ((x & 0x3333333333333333ULL) << 2) | ((x >> 2) & 0x3333333333333333ULL);
    return x;
}
inline u128 revcomp_kmer(u128 v, uint32_t k) {  // rcb, utils.cpp:397-438
    const uint64_t lo = (uint64_t)v, hi = (uint64_t)(v >> 64);
    const u128 r = ((u128)(rev_groups64(lo) ^ 0xaaaaaaaaaaaaaaaaULL) << 64) | (rev_groups64(hi) ^ 0xaaaaaaaaaaaaaaaaULL);
    return r >> (128 - 2 * k);
}

// ---------------------------------------------------------------- sketching --
struct Entry {
    u128 kmer;
    uint32_t minimizer;
    uint8_t count;    // wraps at 256 like the reference's uint8_t (SubSampler.h:24)
    uint8_t pos_min;
    uint8_t seen;
};

// (minimizer, k-mer) -> entry index; linear probing, grows by doubling.
struct KmerIndex {
    std::vector<uint32_t> slot;  // entry index + 1, 0 = empty
    uint64_t mask = 0;
    size_t used = 0;
    static uint64_t hash(uint32_t mn, u128 km) {
        uint64_t x = (uint64_t)km * 0x9E3779B97F4A7C15ULL ^ ((uint64_t)(km >> 64) + mn) * 0xC2B2AE3D27D4EB4FULL;
        x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ULL; x ^= x >> 32;
        return x;
    }
    void init(size_t cap_pow2) { slot.assign(cap_pow2, 0); mask = cap_pow2 - 1; used = 0; }
    void grow(const std::vector<Entry>& es) {
        std::vector<uint32_t> old;
        old.swap(slot);
        init(old.size() * 2);
        for (uint32_t v : old)
            if (v) place(es, v - 1);
    }
    void place(const std::vector<Entry>& es, uint32_t idx) {
        uint64_t p = hash(es[idx].minimizer, es[idx].kmer) & mask;
        while (slot[p]) p = (p + 1) & mask;
        slot[p] = idx + 1; ++used;
    }
    int64_t find(const std::vector<Entry>& es, uint32_t mn, u128 km) const {
        uint64_t p = hash(mn, km) & mask;
        while (slot[p]) {
            const Entry& e = es[slot[p] - 1];
            if (e.kmer == km && e.minimizer == mn) return slot[p] - 1;
            p = (p + 1) & mask;
        }
        return -1;
    }
};

constexpr uint32_t kPlaceholder = 0xffffffffu;   // `order` entry of a k-mer the device abundance pass dropped

struct Builder {
    uint32_t k, m, abundance;
    u128 kmask;
    uint32_t mmask;
    std::vector<Entry> entries;
    KmerIndex index;
    std::vector<std::pair<uint32_t, uint32_t>> order;  // (minimizer, entry index) in insertion order
    spsp_sketch_stats st;

    // Subsampler::handle_superkmer (SubSampler.cpp:243-302) on 2-bit codes.  fl (optional): the device abundance
    // pass's verdict per k-mer of this super-k-mer (spsp_abund.hip) -- a k-mer that will stay below -a is not indexed;
    // the first occurrence of each such k-mer leaves a placeholder, which is what the reference keeps of it (a map
    // entry that is counted, makes its bucket exist and is never usable)
    void add_superkmer(const uint8_t* s, uint32_t len, uint32_t minimizer, bool rev, const uint8_t* fl = nullptr) {
        st.selected_superkmer_number++;
        st.selected_kmer_number += len - k + 1;
        if (len == 2 * k - m) st.count_maximal_skmer++;
        static thread_local std::vector<uint8_t> o;
        o.resize(len);
        if (rev) for (uint32_t t = 0; t < len; ++t) o[t] = (uint8_t)(code_of(s[len - 1 - t]) ^ 2u);
        else for (uint32_t t = 0; t < len; ++t) o[t] = (uint8_t)code_of(s[t]);
        // start positions (oriented) where the m-mer equals the minimizer, ascending
        static thread_local std::vector<uint32_t> occ;
        occ.clear();
        uint32_t mv = 0;
        for (uint32_t t = 0; t < len; ++t) {
            mv = ((mv << 2) | o[t]) & mmask;
            if (t + 1 >= m && mv == minimizer) occ.push_back(t + 1 - m);
        }
        size_t oc = 0;
        u128 kv = 0;
        for (uint32_t t = 0; t < len; ++t) {
            kv = ((kv << 2) | o[t]) & kmask;
            if (t + 1 < k) continue;
            const uint32_t i = t + 1 - k;  // k-mer start
            if (fl && !(fl[i] & 1u)) {
                if (fl[i] & 2u) order.emplace_back(minimizer, kPlaceholder);
                continue;
            }
            while (oc < occ.size() && occ[oc] < i) ++oc;
            // kmerstr.find(minimizer) : first occurrence inside the k-mer, else npos -> (uint8_t)
            const uint8_t pos_min = (oc < occ.size() && occ[oc] + m <= i + k) ? (uint8_t)(occ[oc] - i) : (uint8_t)0xff;
            const int64_t at = index.find(entries, minimizer, kv);
            if (at >= 0) { entries[at].count++; continue; }
            Entry e; e.kmer = kv; e.minimizer = minimizer; e.count = 1; e.pos_min = pos_min; e.seen = 0;
            entries.push_back(e);
            order.emplace_back(minimizer, (uint32_t)entries.size() - 1);
            if ((index.used + 1) * 2 > index.slot.size()) index.grow(entries);
            index.place(entries, (uint32_t)entries.size() - 1);
        }
    }

    bool usable(const Entry& e) const { return !e.seen && e.count >= abundance; }

    // Subsampler::find_next (SubSampler.cpp:566-602): neighbours tried in A,T,C,G order.
    int64_t step(uint32_t mn, u128 from, bool left) {
        static const uint32_t kTry[4] = {0, 2, 1, 3};
        for (uint32_t c : kTry) {
            const u128 nx = left ? ((from >> 2) | ((u128)c << (2 * k - 2))) : (((from << 2) | c) & kmask);
            const int64_t at = index.find(entries, mn, nx);
            if (at >= 0 && usable(entries[at])) { entries[at].seen = 1; return at; }
        }
        return -1;
    }

    // emission half of parse_fasta_test (SubSampler.cpp:458-504): the header line ...
    static void emit_header(uint32_t k, uint32_t m, uint64_t selected_kmers, double rate, std::string& out) {
        char hdr[128];
        const int hl = snprintf(hdr, sizeof hdr, "%llu %llu %llu %f\n", (unsigned long long)(k - 1 + (k - m + 1)),
                                (unsigned long long)m, (unsigned long long)selected_kmers, rate);
        out.append(hdr, hl);
    }
    // ... and the buckets this builder holds (one, when sketch_build_core builds bucket by bucket)
    void emit(std::string& out) {
        // std::map<uint32_t,...> order over buckets, insertion order inside one (ankerl dense map)
        std::stable_sort(order.begin(), order.end(),
                         [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
        const uint32_t full = 2 * k - m, half = k - m;
        std::vector<uint8_t> buf(3 * k + 8), maxcodes;
        std::string text;
        size_t b0 = 0;
        while (b0 < order.size()) {
            size_t b1 = b0;
            const uint32_t mn = order[b0].first;
            while (b1 < order.size() && order[b1].first == mn) ++b1;
            st.actual_minimizer_number++;
            st.seen_kmers_at_reconstruction += b1 - b0;
            for (uint32_t j = 0; j < m; ++j) out.push_back(kNuc[(mn >> (2 * (m - 1 - j))) & 3]);
            maxcodes.clear(); text.clear();
            size_t cursor = b0;  // find_first_kmer: `seen` only ever turns on, so a cursor visits the same k-mers
            for (;;) {
                while (cursor < b1 && (order[cursor].second == kPlaceholder || !usable(entries[order[cursor].second]))) ++cursor;
                if (cursor >= b1) break;
                Entry& start = entries[order[cursor].second];
                start.seen = 1;
                // reconstruct_superkmer (SubSampler.cpp:512-564)
                uint64_t n_left = (uint64_t)half - start.pos_min, n_right = start.pos_min;
                uint32_t L = k + 4, R = L + k;  // [L,R) holds the growing super-k-mer, room for half on each side
                for (uint32_t j = 0; j < k; ++j) buf[L + j] = (uint8_t)((start.kmer >> (2 * (k - 1 - j))) & 3);
                u128 cur = start.kmer;
                while (R - L != full) {
                    if (n_left != 0) {
                        const int64_t at = step(mn, cur, true);
                        n_left -= 1;
                        if (at >= 0) { buf[--L] = (uint8_t)((entries[at].kmer >> (2 * (k - 1))) & 3); }
                        else n_left = 0;
                        if (n_left == 0) cur = start.kmer; else if (at >= 0) cur = entries[at].kmer;
                    } else if (n_right != 0) {
                        const int64_t at = step(mn, cur, false);
                        n_right -= 1;
                        if (at < 0) break;
                        buf[R++] = (uint8_t)(entries[at].kmer & 3);
                        cur = entries[at].kmer;
                    } else break;
                }
                const uint32_t slen = R - L;
                if (slen == full) {
                    st.seen_max_superkmers_at_reconstruction++;
                    maxcodes.insert(maxcodes.end(), buf.begin() + L, buf.begin() + L + half);
                    maxcodes.insert(maxcodes.end(), buf.begin() + L + k, buf.begin() + L + k + half);
                } else {
                    // skmer_str.find(minstr): first m-mer equal to the minimizer
                    uint32_t mv = 0, p = slen;
                    for (uint32_t t = 0; t < slen; ++t) {
                        mv = ((mv << 2) | buf[L + t]) & mmask;
                        if (t + 1 >= m && mv == mn) { p = t + 1 - m; break; }
                    }
                    for (uint32_t t = 0; t < p && t < slen; ++t) text.push_back(kNuc[buf[L + t]]);
                    text.push_back('\n');
                    for (uint32_t t = p + m; t < slen; ++t) text.push_back(kNuc[buf[L + t]]);
                    text.push_back('\n');
                }
                st.seen_superkmers_at_reconstruction++;
            }
            // strCompressor (utils.cpp:48-68), accumulator starting at 0
            std::string blob;
            if (!maxcodes.empty()) {
                const uint8_t mod = (uint8_t)(maxcodes.size() % 4);
                blob.push_back((char)mod);
                uint8_t c = 0;
                for (size_t i = 0; i < maxcodes.size(); ++i) {
                    c = (uint8_t)(c + maxcodes[i]);
                    if ((i + 1) % 4 == 0) { blob.push_back((char)c); c = 0; }
                    c = (uint8_t)(c << 2);
                }
                if (mod != 0) blob.push_back((char)c);
            }
            const uint32_t sz = (uint32_t)blob.size();
            out.append((const char*)&sz, 4);
            out += blob;
            out += text;
            out += "\n\n";
            b0 = b1;
        }
    }
};

// ------------------------------------------------------------- gzip reading --
int inflate_all(const uint8_t* in, size_t n, std::vector<uint8_t>& out) {
    // zstr autodetect (include/zstr.hpp:154-167): gzip or zlib header, else plain
    const bool packed = n >= 2 && ((in[0] == 0x1F && in[1] == 0x8B) ||
                                   (in[0] == 0x78 && (in[1] == 0x01 || in[1] == 0x9C || in[1] == 0xDA)));
    if (!packed) { out.assign(in, in + n); return SPSP_OK; }
    // One inflator per THREAD, reset per member (10 000 sketch files of 3 KB: inflateInit2's 40 KB of state and a zeroed 1 MiB
    // bounce buffer per file were most of the 48 us a file cost its thread), and the output grows in place: the member's ISIZE
    // trailer says how much is coming (a hint only: sizes are taken from what inflate delivers)
    struct Inflator { z_stream zs; bool live = false; ~Inflator() { if (live) inflateEnd(&zs); } };
    static thread_local Inflator I;
    out.clear();
    size_t hint = n * 4 + 64;
    if (n >= 18 && in[0] == 0x1F) { uint32_t isize; memcpy(&isize, in + n - 4, 4); if (isize >= n && isize < (1u << 30)) hint = (size_t)isize + 64; }
    out.resize(hint);
    size_t have = 0, at = 0;
    while (at < n) {  // concatenated members: the inflator starts afresh per member, as zstr does (:198-203)
        if (!I.live) {
            memset(&I.zs, 0, sizeof I.zs);
            if (inflateInit2(&I.zs, 15 + 32) != Z_OK) { set_error("inflateInit2 failed"); return SPSP_ERR_IO; }
            I.live = true;
        } else if (inflateReset2(&I.zs, 15 + 32) != Z_OK) { set_error("inflateReset2 failed"); return SPSP_ERR_IO; }
        z_stream& zs = I.zs;
        zs.avail_in = 0;
        int ret = Z_OK;
        bool truncated = false;
        while (ret != Z_STREAM_END) {
            if (zs.avail_in == 0) {
                if (at >= n) { truncated = true; break; }
                const size_t take = std::min<size_t>(n - at, (size_t)1 << 30);
                zs.next_in = const_cast<Bytef*>(in + at);
                zs.avail_in = (uInt)take;
                at += take;
            }
            if (have == out.size()) out.resize(out.size() * 2 + 4096);
            const size_t room = std::min<size_t>(out.size() - have, (size_t)1 << 30);
            zs.next_out = out.data() + have;
            zs.avail_out = (uInt)room;
            ret = inflate(&zs, Z_NO_FLUSH);
            if (ret != Z_OK && ret != Z_STREAM_END && ret != Z_BUF_ERROR) {
                set_error("inflate failed (%d)", ret);
                return SPSP_ERR_IO;
            }
            have += room - zs.avail_out;
        }
        at -= zs.avail_in;  // bytes not consumed belong to the next member
        if (truncated) break;
    }
    out.resize(have);
    return SPSP_OK;
}

}  // namespace

namespace spsp {

int inflate_all_host(const uint8_t* in, size_t n, std::vector<uint8_t>& out) { return inflate_all(in, n, out); }

// Super-k-mer i's bases come either from the full cleaned sequence (bases + rec_off[rec] + start) or, when the
// ingest ran on the GPU, from a compact buffer holding only the selected super-k-mers (compact + compact_off[i]).
int sketch_build_core(const spsp_params* p, double rate, const uint64_t* rec_off, uint32_t n_rec, const spsp_superkmer* sk,
                      uint64_t n_sk, const uint8_t* bases, const uint8_t* compact, const uint32_t* compact_off,
                      uint8_t** payload, uint64_t* payload_len, spsp_sketch_stats* stats, const uint8_t* kmer_flags) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!payload || !payload_len || (n_rec && !rec_off) || (n_sk && (!sk || (!bases && !(compact && compact_off))))) {
        set_error("NULL argument");
        return SPSP_ERR_ARG;
    }
    // The k-mers of a bucket (one minimizer) meet no k-mer of another: the index is keyed by (minimizer, k-mer), the walk
    // of reconstruct_superkmer stays inside its bucket, buckets are written in minimizer order.  So the super-k-mers are
    // grouped by minimizer (stream order kept inside a group) and every bucket is built and written on its own -- an index
    // that fits a core's cache instead of one over all k-mers of a genome (a 1 Gbp record at -s 100: 10^7 k-mers, 10 us
    // per super-k-mer in one table, 5.0 s), and on several threads when there is enough to do.
    spsp_sketch_stats st;
    memset(&st, 0, sizeof st);
    static const bool dbg_times = getenv("SPSP_DEBUG_BUILD_TIMES") != nullptr;   // analysis: where the builder's time goes (stderr)
    const double bt0 = dbg_times ? now_s() : 0.0;
    uint64_t nb = 0, pos_end = 0, occ = 0;                // occ: k-mer occurrences so far (numbering of kmer_flags)
    uint32_t cur_rec = 0xffffffffu;
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint64_t len = rec_off[r + 1] - rec_off[r];
        if (len >= p->k) st.read_kmer += len - p->k + 1;
    }
    std::vector<std::pair<uint32_t, uint32_t>> by_mn;     // (minimizer, super-k-mer)
    std::vector<uint64_t> occ_of;                         // first k-mer occurrence of every super-k-mer (kmer_flags)
    if (n_sk > 0xfffffff0ull) { set_error("too many super-k-mers for one sketch"); return SPSP_ERR_OVERFLOW; }
    by_mn.reserve((size_t)n_sk);
    if (kmer_flags) occ_of.reserve((size_t)n_sk);
    for (uint64_t i = 0; i < n_sk; ++i) {
        const spsp_superkmer& e = sk[i];
        if (e.rec >= n_rec || e.len < p->k || e.start + e.len > rec_off[e.rec + 1] - rec_off[e.rec]) {
            set_error("super-k-mer %llu is outside its record", (unsigned long long)i);
            return SPSP_ERR_ARG;
        }
        // nb_mmer_selected bookkeeping (SubSampler.cpp:410-424, 445): a pure function of the stream
        if (e.rec != cur_rec) { cur_rec = e.rec; pos_end = 0; }
        const uint64_t rlen = rec_off[e.rec + 1] - rec_off[e.rec];
        if (e.start + e.len == rlen) nb -= p->m - 1;  // the tail call :441-450
        else {
            if (e.start + p->m - 2 > pos_end) {
                if (pos_end > 0) nb -= p->m - 1;
                nb += e.len;
                nb -= p->k - p->m;
            } else nb += e.start + e.len - (pos_end + 1);
            pos_end = e.start + e.len - 1;
        }
        by_mn.emplace_back(e.minimizer, (uint32_t)i);
        if (kmer_flags) occ_of.push_back(occ);
        st.selected_kmer_number += e.len - p->k + 1;
        occ += e.len - p->k + 1;
    }
    nb -= p->m - 1;  // SubSampler.cpp:458
    st.nb_mmer_selected = nb;
    // grouped by minimizer, stream order kept inside a group: two stable counting passes over 16 bits each (a comparison sort of
    // the 8 x 10^5 super-k-mers of a 4 Gbp metagenome segment was 0.1 s on one thread in front of the threaded part)
    if (by_mn.size() > 4096) {
        std::vector<std::pair<uint32_t, uint32_t>> tmp(by_mn.size());
        std::vector<uint32_t> cnt(65537);
        for (int pass = 0; pass < 2; ++pass) {
            const int sh = 16 * pass;
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (const auto& e : by_mn) ++cnt[((e.first >> sh) & 0xffffu) + 1];
            for (size_t i = 1; i < cnt.size(); ++i) cnt[i] += cnt[i - 1];
            for (const auto& e : by_mn) tmp[cnt[(e.first >> sh) & 0xffffu]++] = e;
            by_mn.swap(tmp);
        }
    } else
        std::stable_sort(by_mn.begin(), by_mn.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
    struct Bucket { size_t first, last; std::string text; spsp_sketch_stats st; };
    std::vector<Bucket> buckets;
    for (size_t a = 0; a < by_mn.size();) {
        size_t z = a;
        while (z < by_mn.size() && by_mn[z].first == by_mn[a].first) ++z;
        buckets.push_back(Bucket{a, z, std::string(), spsp_sketch_stats{}});
        a = z;
    }
    const double bt1 = dbg_times ? now_s() : 0.0;
    std::vector<uint32_t> todo(buckets.size());           // largest first: the threads finish together
    for (uint32_t i = 0; i < todo.size(); ++i) todo[i] = i;
    std::sort(todo.begin(), todo.end(), [&](uint32_t a, uint32_t b) { return buckets[a].last - buckets[a].first > buckets[b].last - buckets[b].first; });
    std::atomic<uint32_t> next{0};
    auto work = [&]() {
        for (;;) {
            const uint32_t t = next.fetch_add(1);
            if (t >= todo.size()) return;
            Bucket& B = buckets[todo[t]];
            Builder b;
            b.k = p->k; b.m = p->m; b.abundance = p->abundance;
            b.kmask = (((u128)1) << (2 * p->k)) - 1;
            b.mmask = (1u << (2 * p->m)) - 1;
            memset(&b.st, 0, sizeof b.st);
            b.index.init(1024);
            for (size_t x = B.first; x < B.last; ++x) {
                const uint32_t i = by_mn[x].second;
                const spsp_superkmer& e = sk[i];
                const uint8_t* src = compact ? compact + compact_off[i] : bases + rec_off[e.rec] + e.start;
                b.add_superkmer(src, e.len, e.minimizer, e.rev != 0, kmer_flags ? kmer_flags + occ_of[i] : nullptr);
            }
            b.emit(B.text);                               // (nothing when every k-mer of the bucket was dropped without a trace: the bucket does not exist)
            B.st = b.st;
        }
    };
    // (the file pipeline builds the sketches of different files on its own worker threads: threads of its own only for a
    // sketch that is large by itself)
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned n_thr = n_sk >= 20000 ? std::min<unsigned>(std::min<unsigned>(n_sk >= 400000 ? 16u : 8u, hw), (unsigned)std::max<size_t>(1, buckets.size())) : 1u;
    if (n_thr <= 1) work();
    else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < n_thr; ++t) pool.emplace_back(work);
        for (auto& th : pool) th.join();
    }
    const double bt2 = dbg_times ? now_s() : 0.0;
    std::string out;
    Builder::emit_header(p->k, p->m, st.selected_kmer_number, rate, out);
    for (const Bucket& B : buckets) {
        out += B.text;
        st.selected_superkmer_number += B.st.selected_superkmer_number;
        st.count_maximal_skmer += B.st.count_maximal_skmer;
        st.actual_minimizer_number += B.st.actual_minimizer_number;
        st.seen_kmers_at_reconstruction += B.st.seen_kmers_at_reconstruction;
        st.seen_superkmers_at_reconstruction += B.st.seen_superkmers_at_reconstruction;
        st.seen_max_superkmers_at_reconstruction += B.st.seen_max_superkmers_at_reconstruction;
    }
    *payload = (uint8_t*)malloc(out.size() + 1);
    if (!*payload) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    memcpy(*payload, out.data(), out.size());
    *payload_len = out.size();
    if (stats) *stats = st;
    if (dbg_times) fprintf(stderr, "[spsp build] %llu super-k-mers, %zu buckets, %u threads: group by minimizer %.1f ms, buckets %.1f ms, join %.1f ms\n",
                           (unsigned long long)n_sk, buckets.size(), n_thr, (bt1 - bt0) * 1e3, (bt2 - bt1) * 1e3, (now_s() - bt2) * 1e3);
    return SPSP_OK;
}

// What the device builder (spsp_build.hip) leaves to the host: the counters that are a pure function of the scan's stream
// (the same lines as in sketch_build_core above) and the header line.
int sketch_stream_stats(const spsp_params* p, const uint64_t* rec_off, uint32_t n_rec, const spsp_superkmer* sk, uint64_t n_sk, spsp_sketch_stats* st_out) {
    spsp_sketch_stats st;
    memset(&st, 0, sizeof st);
    uint64_t nb = 0, pos_end = 0;
    uint32_t cur_rec = 0xffffffffu;
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint64_t len = rec_off[r + 1] - rec_off[r];
        if (len >= p->k) st.read_kmer += len - p->k + 1;
    }
    for (uint64_t i = 0; i < n_sk; ++i) {
        const spsp_superkmer& e = sk[i];
        if (e.rec >= n_rec || e.len < p->k || e.start + e.len > rec_off[e.rec + 1] - rec_off[e.rec]) {
            set_error("super-k-mer %llu is outside its record", (unsigned long long)i);
            return SPSP_ERR_ARG;
        }
        if (e.rec != cur_rec) { cur_rec = e.rec; pos_end = 0; }
        const uint64_t rlen = rec_off[e.rec + 1] - rec_off[e.rec];
        if (e.start + e.len == rlen) nb -= p->m - 1;
        else {
            if (e.start + p->m - 2 > pos_end) {
                if (pos_end > 0) nb -= p->m - 1;
                nb += e.len;
                nb -= p->k - p->m;
            } else nb += e.start + e.len - (pos_end + 1);
            pos_end = e.start + e.len - 1;
        }
        st.selected_kmer_number += e.len - p->k + 1;
        st.selected_superkmer_number++;
        if (e.len == 2 * p->k - p->m) st.count_maximal_skmer++;
    }
    nb -= p->m - 1;
    st.nb_mmer_selected = nb;
    *st_out = st;
    return SPSP_OK;
}
void sketch_header_line(uint32_t k, uint32_t m, uint64_t selected_kmers, double rate, std::string& out) { Builder::emit_header(k, m, selected_kmers, rate, out); }

// structure of one payload for the GPU decoder (spsp_decode.hip): header (Comparator.cpp:23-37) and, per bucket,
// [m ASCII][u32 n][blob][lines]["\n\n"] (:186-260).  Every offset it hands to the device is checked against `len` here.
int sketch_parse_structure_host(const uint8_t* payload, uint64_t len, ParsedSketch* P) {
    const uint8_t* nl = (payload && len) ? (const uint8_t*)memchr(payload, '\n', len) : nullptr;
    if (!nl) { set_error("sketch has no header line"); return SPSP_ERR_FORMAT; }
    char* endp = nullptr;
    const std::string header((const char*)payload, nl - payload);
    const long skm = strtol(header.c_str(), &endp, 10);
    const long mm = strtol(endp, &endp, 10);
    if (skm <= 0 || skm > 126 || mm <= 0 || mm > 15 || (skm + mm) / 2 > 63 || (skm + mm) / 2 < mm) { set_error("bad sketch header '%.60s'", header.c_str()); return SPSP_ERR_FORMAT; }
    const uint32_t m = (uint32_t)mm, k = (uint32_t)((skm + mm) / 2), half = (uint32_t)((skm - mm) / 2);
    P->k = k; P->m = m;
    uint64_t pos = (uint64_t)(nl - payload) + 1;
    uint64_t out = 0;
    auto push = [&](uint64_t off, uint32_t mn, uint32_t info, uint64_t count) {
        if (count == 0) return;
        if (out + count > 0xfffffff0ull) { P->standard = false; return; }
        P->desc.push_back(DecDesc{off, mn, info, (uint32_t)out, 0});
        out += count;
    };
    while (pos + m <= len) {
        uint32_t mn = 0;
        for (uint32_t j = 0; j < m; ++j) mn = (mn << 2) | code_of(payload[pos + j]);
        pos += m;
        uint32_t nbytes = 0;
        if (pos + 4 > len) break;
        memcpy(&nbytes, payload + pos, 4);
        pos += 4;
        if (pos + nbytes > len) { set_error("bucket blob runs past the end of the sketch"); return SPSP_ERR_FORMAT; }
        uint64_t seq_len = 0;
        if (nbytes) {
            if (payload[pos] != 0) P->standard = false;           // a partial last byte: never written by the sketcher (k, m odd)
            seq_len = (uint64_t)(nbytes - 1) * 4;
        }
        if (half > 0) {
            if ((2 * half) % 4 != 0) P->standard = false;         // k - m odd (never from bin/sub_sampler, which forces k and m odd, SubSampler.cpp:732-741; possible through spsp_sketch_build_host): a blob byte then straddles two super-k-mers -- host decoder
            for (uint64_t i = 0; (i + 1) * 2 * half <= seq_len; ++i) push(pos + 1 + i * (half / 2), mn, 0u, k - m + 1);
        } else if (seq_len == 0) {
            push(pos, mn, 2u, 1);                                  // k == m: the bare minimizer is one k-mer (Comparator.cpp:88-90,193-198)
        }
        pos += nbytes;
        for (;;) {                                                 // "prefix\nsuffix\n" until an empty pair (:226-260)
            if (pos >= len) break;
            const uint8_t* e1 = (const uint8_t*)memchr(payload + pos, '\n', len - pos);
            const uint64_t s1 = pos, l1 = e1 ? (uint64_t)(e1 - payload) - pos : len - pos;
            pos = e1 ? s1 + l1 + 1 : len;
            const uint8_t* e2 = pos < len ? (const uint8_t*)memchr(payload + pos, '\n', len - pos) : nullptr;
            const uint64_t s2 = pos, l2 = pos < len ? (e2 ? (uint64_t)(e2 - payload) - pos : len - pos) : 0;
            pos = e2 ? s2 + l2 + 1 : len;
            if (l1 == 0 && l2 == 0) break;
            if (!e1 || l1 > 255 || l2 > 255 || s2 != s1 + l1 + 1) { P->standard = false; continue; }
            const uint64_t total = l1 + m + l2;
            push(s1, mn, 1u | ((uint32_t)l1 << 2) | ((uint32_t)l2 << 10), total >= k ? total - k + 1 : 0);
        }
    }
    P->n_keys = out;
    return SPSP_OK;
}

}  // namespace spsp

extern "C" {

// Subsampler::compute_threshold (SubSampler.cpp:622-631) + SubSampler.h:79-83
uint64_t spsp_threshold_host(uint32_t k, uint32_t m, double sampling_rate) {
    if (!(sampling_rate > 1)) return ~0ULL;
    const uint64_t w = (uint64_t)k - m + 1;
    const long double frac = (long double)1 / sampling_rate;
    const long double root = powl((long double)1 - frac, (long double)1 / w);
    const long double scaled = ((long double)1 - root) * ((uint64_t)1 << 63);
    return (uint64_t)scaled * 2;
}

int spsp_fasta_clean_host(const char* text, uint64_t n, uint8_t** bases, uint64_t** rec_off, uint32_t* n_rec) {
    if (!bases || !rec_off || !n_rec || (n && !text)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    // keep[c] = upper-cased base for acgtACGT, 0 for everything else (clean_dna, utils.cpp:675-702)
    struct Keep {
        uint8_t t[256];
        Keep() {
            memset(t, 0, sizeof t);
            for (const char* q = "ACGT"; *q; ++q) { t[(uint8_t)*q] = (uint8_t)*q; t[(uint8_t)(*q + 32)] = (uint8_t)*q; }
        }
    };
    static const Keep keep_tab;
    const uint8_t* keep = keep_tab.t;
    std::vector<uint64_t> off;
    uint8_t* out = (uint8_t*)malloc((size_t)n + 64);
    if (!out) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    uint64_t w = 0, pos = 0;
    bool at_end = false;
    // SubSampler.cpp:334-348 + getLineFasta utils.cpp:706-718: every turn drops
    // one line, then swallows lines up to the next one starting with '>'.
    while (!at_end) {
        off.push_back(w);
        const char* nl = pos < n ? (const char*)memchr(text + pos, '\n', n - pos) : nullptr;
        if (!nl) { pos = n; at_end = true; } else pos = (uint64_t)(nl - text) + 1;
        while (!at_end) {
            if (pos >= n) { at_end = true; break; }
            const uint8_t c0 = (uint8_t)text[pos];
            if (c0 == '>' || c0 == 0xFF) break;  // (char)peek() == EOF aliasing for 0xFF
            const char* e = (const char*)memchr(text + pos, '\n', n - pos);
            const uint64_t stop = e ? (uint64_t)(e - text) : n;
            for (uint64_t i = pos; i < stop; ++i) {
                const uint8_t b = keep[(uint8_t)text[i]];
                out[w] = b;
                w += (b != 0);
            }
            if (!e) { pos = n; at_end = true; } else pos = stop + 1;
        }
    }
    off.push_back(w);
    *bases = out;
    *rec_off = dup_vec(off);
    *n_rec = (uint32_t)(off.size() - 1);
    if (!*rec_off) { free(out); set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    return SPSP_OK;
}

int spsp_sketch_build_host(const spsp_params* p, double rate, const uint8_t* bases, const uint64_t* rec_off,
                           uint32_t n_rec, const spsp_superkmer* sk, uint64_t n_sk, uint8_t** payload,
                           uint64_t* payload_len, spsp_sketch_stats* stats) {
    if (n_sk && !bases) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    return spsp::sketch_build_core(p, rate, rec_off, n_rec, sk, n_sk, bases, nullptr, nullptr, payload, payload_len, stats, nullptr);
}

int spsp_sketch_parse_host(const uint8_t* payload, uint64_t len, uint32_t* k_out, uint32_t* m_out,
                           uint32_t** minimizer, uint64_t** kmer_lo, uint64_t** kmer_hi, uint64_t* n_out) {
    if (!payload || !k_out || !m_out || !minimizer || !kmer_lo || !kmer_hi || !n_out) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    // header "<2k-m> <m> <n> <rate>\n" (Comparator.cpp:23-37)
    const uint8_t* nl = (const uint8_t*)memchr(payload, '\n', len);
    if (!nl) { set_error("sketch has no header line"); return SPSP_ERR_FORMAT; }
    char* endp = nullptr;
    const std::string header((const char*)payload, nl - payload);
    const long skm = strtol(header.c_str(), &endp, 10);
    const long mm = strtol(endp, &endp, 10);
    // (range checks first: strtol saturates at LONG_MAX on garbage and the sums below must not overflow)
    if (skm <= 0 || skm > 126 || mm <= 0 || mm > 15 || (skm + mm) / 2 > 63 || (skm + mm) / 2 < mm) { set_error("bad sketch header '%.60s'", header.c_str()); return SPSP_ERR_FORMAT; }
    const uint32_t m = (uint32_t)mm, k = (uint32_t)((skm + mm) / 2), half = (uint32_t)((skm - mm) / 2);
    const u128 kmask = (((u128)1) << (2 * k)) - 1;
    struct Key { uint32_t mn; uint64_t hi, lo; };
    std::vector<Key> keys;
    std::vector<uint8_t> seq;
    auto push_kmers = [&](const std::vector<uint8_t>& s, size_t from, size_t count_limit, uint32_t mn) {
        // canonical k-mers of s[from..], at most count_limit of them
        u128 kv = 0;
        size_t made = 0;
        for (size_t t = from; t < s.size() && made < count_limit; ++t) {
            kv = ((kv << 2) | s[t]) & kmask;
            if (t + 1 - from < k) continue;
            const u128 rc = revcomp_kmer(kv, k);
            const u128 c = kv < rc ? kv : rc;
            keys.push_back(Key{mn, (uint64_t)(c >> 64), (uint64_t)c});
            ++made;
        }
    };
    uint64_t pos = (uint64_t)(nl - payload) + 1;
    while (pos + m <= len) {
        uint32_t mn = 0;
        for (uint32_t j = 0; j < m; ++j) mn = (mn << 2) | code_of(payload[pos + j]);
        pos += m;
        uint32_t nbytes = 0;
        if (pos + 4 > len) break;
        memcpy(&nbytes, payload + pos, 4);
        pos += 4;
        if (pos + nbytes > len) { set_error("bucket blob runs past the end of the sketch"); return SPSP_ERR_FORMAT; }
        // strDecompressor (utils.cpp:71-111)
        seq.clear();
        if (nbytes) {
            const uint8_t mod = payload[pos];
            const uint64_t last = (mod == 0) ? nbytes : nbytes - 1;
            for (uint64_t i = 1; i < last; ++i) {
                const uint8_t b = payload[pos + i];
                seq.push_back((b >> 6) & 3); seq.push_back((b >> 4) & 3); seq.push_back((b >> 2) & 3); seq.push_back(b & 3);
            }
            if (mod != 0 && last >= 1) {
                uint8_t b = payload[pos + last];
                uint8_t f[4] = {0, 0, 0, 0};
                for (int i = 0; i < (int)(mod & 3) + 1; ++i) { f[(mod & 3) - i] = b & 3; b >>= 2; }
                for (int i = 0; i < (int)(mod & 3); ++i) seq.push_back(f[i]);
            }
        }
        pos += nbytes;
        // inject_minimizer (Comparator.cpp:78-92) + maximal walk (:196-225): every
        // 2(k-m) stored bases are one maximal super-k-mer = k-m+1 k-mers
        if (half > 0) {
            std::vector<uint8_t> sk(2 * half + m);
            for (size_t i = 0; i + 2 * half <= seq.size(); i += 2 * half) {
                for (uint32_t j = 0; j < half; ++j) sk[j] = seq[i + j];
                for (uint32_t j = 0; j < m; ++j) sk[half + j] = (mn >> (2 * (m - 1 - j))) & 3;
                for (uint32_t j = 0; j < half; ++j) sk[half + m + j] = seq[i + half + j];
                push_kmers(sk, 0, k - m + 1, mn);
            }
        } else if (seq.empty()) {
            // k == m: inject_minimizer returns the bare minimizer for an empty blob and, being k long,
            // it is walked as one k-mer (Comparator.cpp:88-90,193-198)
            std::vector<uint8_t> sk(m);
            for (uint32_t j = 0; j < m; ++j) sk[j] = (mn >> (2 * (m - 1 - j))) & 3;
            push_kmers(sk, 0, 1, mn);
        }
        // non-maximal super-k-mers: "prefix\nsuffix\n" until an empty pair (:226-260)
        for (;;) {
            if (pos >= len) break;
            const uint8_t* e1 = (const uint8_t*)memchr(payload + pos, '\n', len - pos);
            const uint64_t s1 = pos, l1 = e1 ? (uint64_t)(e1 - payload) - pos : len - pos;
            pos = e1 ? s1 + l1 + 1 : len;
            const uint8_t* e2 = pos < len ? (const uint8_t*)memchr(payload + pos, '\n', len - pos) : nullptr;
            const uint64_t s2 = pos, l2 = pos < len ? (e2 ? (uint64_t)(e2 - payload) - pos : len - pos) : 0;
            pos = e2 ? s2 + l2 + 1 : len;
            if (l1 == 0 && l2 == 0) break;
            std::vector<uint8_t> sk;
            sk.reserve(l1 + m + l2);
            for (uint64_t j = 0; j < l1; ++j) sk.push_back((uint8_t)code_of(payload[s1 + j]));
            for (uint32_t j = 0; j < m; ++j) sk.push_back((mn >> (2 * (m - 1 - j))) & 3);
            for (uint64_t j = 0; j < l2; ++j) sk.push_back((uint8_t)code_of(payload[s2 + j]));
            push_kmers(sk, 0, (size_t)-1, mn);
        }
    }
    // distinct canonical k-mers per bucket == distinct (minimizer, k-mer) keys
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
        if (a.mn != b.mn) return a.mn < b.mn;
        if (a.hi != b.hi) return a.hi < b.hi;
        return a.lo < b.lo;
    });
    keys.erase(std::unique(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.mn == b.mn && a.hi == b.hi && a.lo == b.lo; }), keys.end());
    const size_t n = keys.size();
    uint32_t* mn = (uint32_t*)malloc(std::max<size_t>(1, n) * 4);
    uint64_t* lo = (uint64_t*)malloc(std::max<size_t>(1, n) * 8);
    uint64_t* hi = (uint64_t*)malloc(std::max<size_t>(1, n) * 8);
    if (!mn || !lo || !hi) { free(mn); free(lo); free(hi); set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    for (size_t i = 0; i < n; ++i) { mn[i] = keys[i].mn; lo[i] = keys[i].lo; hi[i] = keys[i].hi; }
    *minimizer = mn; *kmer_lo = lo; *kmer_hi = hi; *n_out = n; *k_out = k; *m_out = m;
    return SPSP_OK;
}

// The N-way merge starts by reading every file's first minimizer into ONE shared buffer, without an end-of-file
// check (increment_files INITIALIZATION, Comparator.cpp:316-319; buffer = m times 'A', :294).  A sketch with no
// bucket therefore leaves the buffer as the previous file filled it and enters the merge with that minimizer and an
// empty blob; inject_minimizer turns an empty blob into the bare minimizer (:88-90), which is dropped when m < k
// (:193-195) but IS a k-mer when k == m.  So with k == m an empty sketch holds one phantom k-mer that depends on
// its predecessor in the file list.  This emulates that read for one sketch, in file order.
int spsp_sketch_chain_host(const uint8_t* payload, uint64_t len, uint32_t k, uint32_t m, char* read_buffer, int* has_key,
                           uint32_t* minimizer, uint64_t* kmer_lo, uint64_t* kmer_hi) {
    if (!payload || !read_buffer || !has_key || !minimizer || !kmer_lo || !kmer_hi) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *has_key = 0;
    const uint8_t* nl = (const uint8_t*)memchr(payload, '\n', len);
    if (!nl) { set_error("sketch has no header line"); return SPSP_ERR_FORMAT; }
    const uint64_t body = len - (uint64_t)(nl + 1 - payload);
    const uint64_t got = body < m ? body : m;
    memcpy(read_buffer, nl + 1, (size_t)got);          // istream::read stores what it could read
    if (got == m || k != m) return SPSP_OK;            // a real first bucket, or a phantom that is dropped (m < k)
    uint32_t mn = 0;
    u128 kv = 0;
    for (uint32_t j = 0; j < m; ++j) { const uint32_t c = code_of((uint8_t)read_buffer[j]); mn = (mn << 2) | c; kv = (kv << 2) | c; }
    const u128 rc = revcomp_kmer(kv, k);
    const u128 c = kv < rc ? kv : rc;
    *minimizer = mn; *kmer_lo = (uint64_t)c; *kmer_hi = (uint64_t)(c >> 64);
    *has_key = 1;
    return SPSP_OK;
}

}  // extern "C"

namespace {
// XXH64 of one little-endian 64-bit word, seed 1312: the host's copy of xxh64_u64 (spsp_device.h; Subsampler::unrevhash,
// SubSampler.cpp:64-67 -> include/xxhash64.h:100-150)
inline uint64_t rotl64_host(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }
uint64_t xxh64_u64_host(uint64_t x) {
    constexpr uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL, P3 = 1609587929392839161ULL,
                       P4 = 9650029242287828579ULL, P5 = 2870177450012600261ULL;
    uint64_t h = 1312ULL + P5 + 8ULL;
    h ^= rotl64_host(x * P2, 31) * P1;
    h = rotl64_host(h, 27) * P1 + P4;
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}

// the four header fields "<2k-m> <m> <n> <rate>\n" (SubSampler.cpp:458-470 writes them, Comparator.cpp:23-37 reads them);
// *body = offset of the first byte behind the header line
int sketch_header_fields(const uint8_t* payload, uint64_t len, uint32_t* k, uint32_t* m, uint64_t* n_kmers, double* rate, uint64_t* body) {
    const uint8_t* nl = (payload && len) ? (const uint8_t*)memchr(payload, '\n', len) : nullptr;
    if (!nl) { set_error("sketch has no header line"); return SPSP_ERR_FORMAT; }
    const std::string header((const char*)payload, nl - payload);
    char* e = nullptr;
    const long skm = strtol(header.c_str(), &e, 10);
    const long mm = strtol(e, &e, 10);
    if (skm <= 0 || skm > 126 || mm <= 0 || mm > 15 || (skm + mm) / 2 > 63 || (skm + mm) / 2 < mm) { set_error("bad sketch header '%.60s'", header.c_str()); return SPSP_ERR_FORMAT; }
    char* e3 = nullptr;
    const unsigned long long cnt = strtoull(e, &e3, 10);
    if (e3 == e) { set_error("sketch header '%.60s' has no k-mer count", header.c_str()); return SPSP_ERR_FORMAT; }
    char* e4 = nullptr;
    const double r = strtod(e3, &e4);                              // (-s is a float, printed with %f: strtod, not stoi)
    if (e4 == e3 || !(r == r)) { set_error("sketch header '%.60s' has no sampling rate", header.c_str()); return SPSP_ERR_FORMAT; }
    *m = (uint32_t)mm; *k = (uint32_t)((skm + mm) / 2); *n_kmers = cnt; *rate = r;
    if (body) *body = (uint64_t)(nl - payload) + 1;
    return SPSP_OK;
}
}  // namespace

extern "C" {

int spsp_sketch_header_host(const uint8_t* payload, uint64_t len, uint32_t* k, uint32_t* m, uint64_t* n_kmers, double* rate) {
    if (!payload || !k || !m || !n_kmers || !rate) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    return sketch_header_fields(payload, len, k, m, n_kmers, rate, nullptr);
}

int spsp_sketch_downsample_host(const uint8_t* payload, uint64_t len, double rate, uint8_t** out, uint64_t* out_len) {
    if (!payload || !out || !out_len) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *out = nullptr; *out_len = 0;
    if (!(rate > 0)) { set_error("sampling rate %g: must be positive", rate); return SPSP_ERR_ARG; }
    uint32_t k = 0, m = 0; uint64_t n_old = 0, pos = 0; double own = 0;
    int rc = sketch_header_fields(payload, len, &k, &m, &n_old, &own, &pos);
    if (rc) return rc;
    // rates are compared as the thresholds they stand for, not as the floats the header prints
    const uint64_t thr_own = spsp_threshold_host(k, m, own), thr = spsp_threshold_host(k, m, rate);
    if (thr > thr_own) { set_error("cannot upsample: the sketch was made at rate %g, asked for %g", own, rate); return SPSP_ERR_ARG; }
    auto give = [&](const std::string& s) {
        *out = (uint8_t*)malloc(s.size() + 1);
        if (!*out) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
        memcpy(*out, s.data(), s.size());
        *out_len = s.size();
        return SPSP_OK;
    };
    if (thr == thr_own) return give(std::string((const char*)payload, (size_t)len));   // already there: the sketch as it is
    // the bucket walk of sketch_parse_structure_host: [m ASCII][u32 n][blob]["prefix\nsuffix\n" ...]["\n\n"]; a bucket stays, byte
    // for byte and in its place, iff its minimizer passes
    const std::string old_header((const char*)payload, (size_t)pos);
    std::string body;
    while (pos + m <= len) {
        const uint64_t start = pos;
        uint32_t mn = 0;
        for (uint32_t j = 0; j < m; ++j) mn = (mn << 2) | code_of(payload[pos + j]);
        pos += m;
        uint32_t nbytes = 0;
        if (pos + 4 > len) break;
        memcpy(&nbytes, payload + pos, 4);
        pos += 4;
        if (pos + nbytes > len) { set_error("bucket blob runs past the end of the sketch"); return SPSP_ERR_FORMAT; }
        pos += nbytes;
        for (;;) {
            if (pos >= len) break;
            const uint8_t* e1 = (const uint8_t*)memchr(payload + pos, '\n', len - pos);
            const uint64_t l1 = e1 ? (uint64_t)(e1 - payload) - pos : len - pos;
            pos = e1 ? pos + l1 + 1 : len;
            const uint8_t* e2 = pos < len ? (const uint8_t*)memchr(payload + pos, '\n', len - pos) : nullptr;
            const uint64_t l2 = pos < len ? (e2 ? (uint64_t)(e2 - payload) - pos : len - pos) : 0;
            pos = e2 ? pos + l2 + 1 : len;
            if (l1 == 0 && l2 == 0) break;
        }
        if (xxh64_u64_host(mn) <= thr) body.append((const char*)payload + start, (size_t)(pos - start));
    }
    // the header's third field is read by nobody (Comparator.cpp:31): the DISTINCT keys the kept buckets decode to
    uint64_t n_keys = 0;
    {
        const std::string probe = old_header + body;
        uint32_t kk = 0, mm = 0; uint32_t* a = nullptr; uint64_t *b = nullptr, *c = nullptr;
        if ((rc = spsp_sketch_parse_host((const uint8_t*)probe.data(), probe.size(), &kk, &mm, &a, &b, &c, &n_keys))) return rc;
        free(a); free(b); free(c);
    }
    std::string res;
    spsp::sketch_header_line(k, m, n_keys, rate, res);
    res += body;
    return give(res);
}

// A sketch from keys: the writer the selection ends in.  One bucket per distinct minimizer, ascending: the minimizer's m letters, a
// zero blob size (no maximal super-k-mers), per key ONE non-maximal super-k-mer of exactly k bases as "prefix\nsuffix\n", and the
// closing "\n\n".  A key's k-mer is written in the orientation in which the minimizer's value occurs literally -- the canonical one
// when both hold it -- split at the first occurrence there: the reader (the pair walk above, Comparator.cpp:226-260) puts the
// minimizer back between the two halves and finds exactly one k-mer per pair, whose canonical form is the key's.
int spsp_sketch_from_keys_host(uint32_t k, uint32_t m, double rate, const uint32_t* minimizer, const uint64_t* kmer_lo, const uint64_t* kmer_hi,
                               uint64_t n, uint8_t** payload, uint64_t* len) {
    if (!payload || !len || (n && (!minimizer || !kmer_lo))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *payload = nullptr; *len = 0;
    if (k < 1 || k > 63 || m < 1 || m > 15 || m > k) { set_error("k=%u m=%u: needs 1 <= m <= 15, m <= k <= 63", k, m); return SPSP_ERR_ARG; }
    if (k == m) { set_error("a sketch cannot be written from keys when k == m (k = m = %u): a bucket's key is its bare minimizer", k); return SPSP_ERR_ARG; }
    if (k > 32 && n && !kmer_hi) { set_error("NULL argument: k > 32 needs kmer_hi"); return SPSP_ERR_ARG; }
    const uint32_t mmask = (uint32_t)((1ull << (2 * m)) - 1);
    std::string out;
    spsp::sketch_header_line(k, m, n, rate, out);
    out.reserve(out.size() + (size_t)n * (k - m + 2) + 64);
    char word[64];
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t mn = minimizer[i];
        const u128 km = ((u128)(k > 32 ? kmer_hi[i] : 0) << 64) | kmer_lo[i];
        if (i) {
            const u128 before = ((u128)(k > 32 ? kmer_hi[i - 1] : 0) << 64) | kmer_lo[i - 1];
            if (minimizer[i - 1] > mn || (minimizer[i - 1] == mn && before >= km)) {
                set_error("key %llu does not come strictly after key %llu: keys must be strictly increasing by (minimizer, kmer_hi, kmer_lo)",
                          (unsigned long long)i, (unsigned long long)(i - 1));
                return SPSP_ERR_ARG;
            }
        }
        // the first place the minimizer's value stands at, in the k-mer as the key holds it (canonical), else in its reverse complement
        u128 as = km;
        int at = -1;
        if ((mn & ~mmask) == 0 && (k == 64 || (km >> (2 * k)) == 0)) {
            for (int turn = 0; turn < 2 && at < 0; ++turn) {
                if (turn) as = revcomp_kmer(km, k);
                for (uint32_t q = 0; q + m <= k; ++q)
                    if (((uint32_t)(as >> (2 * (k - m - q))) & mmask) == mn) { at = (int)q; break; }
            }
        }
        if (at < 0) {
            set_error("key %llu: its minimizer (%u) occurs in neither orientation of its k-mer", (unsigned long long)i, mn);
            return SPSP_ERR_ARG;
        }
        if (i == 0 || minimizer[i - 1] != mn) {
            if (i) out.append("\n\n", 2);
            for (uint32_t j = 0; j < m; ++j) word[j] = kNuc[(mn >> (2 * (m - 1 - j))) & 3u];
            out.append(word, m);
            out.append(4, '\0');                               // the blob's size: no maximal super-k-mers
        }
        for (uint32_t j = 0; j < k; ++j) word[j] = kNuc[(uint32_t)(as >> (2 * (k - 1 - j))) & 3u];
        out.append(word, (size_t)at);
        out.push_back('\n');
        out.append(word + at + m, (size_t)(k - m - (uint32_t)at));
        out.push_back('\n');
    }
    if (n) out.append("\n\n", 2);
    *payload = (uint8_t*)malloc(out.size() + 1);
    if (!*payload) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    memcpy(*payload, out.data(), out.size());
    *len = out.size();
    return SPSP_OK;
}

// The band of holder counts a word stands for, among R references: the text bin/comparator -S / -E and the Python interface share.
// <t> is read as -c and -P read theirs (bin/comparator's parse_fraction): a decimal in (0, 1] with at most six digits behind the
// point, as TEXT into num / 10^digits; core_min = ceil(num * R / den) as the prevalence pass computes it.  An empty band is [1, 0]
int spsp_select_band_host(const char* what, uint32_t R, uint32_t* h_min, uint32_t* h_max) {
    if (!what || !h_min || !h_max) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *h_min = 1; *h_max = 0;
    if (R == 0) { set_error("a band of holder counts needs at least one reference"); return SPSP_ERR_ARG; }
    auto fraction = [](const char* t, uint64_t* num, uint64_t* den) {
        if ((t[0] != '0' && t[0] != '1') || (t[1] != 0 && t[1] != '.')) return false;
        uint64_t a = (uint64_t)(t[0] - '0'), d = 1;
        if (t[1] == '.') {
            const char* f = t + 2;
            if (*f == 0) return false;
            for (; *f; ++f) {
                if (*f < '0' || *f > '9' || d >= 1000000) return false;
                a = a * 10 + (uint64_t)(*f - '0'); d *= 10;
            }
        }
        if (a < 1 || a > d) return false;
        *num = a; *den = d;
        return true;
    };
    auto plain = [](const char* b, const char* e, uint32_t* v) {     // [b, e): decimal digits, below 2^32
        if (b == e || e - b > 10) return false;
        uint64_t x = 0;
        for (const char* q = b; q < e; ++q) { if (*q < '0' || *q > '9') return false; x = x * 10 + (uint64_t)(*q - '0'); }
        if (x > 0xffffffffull) return false;
        *v = (uint32_t)x;
        return true;
    };
    const std::string w(what);
    if (w == "union" || w == "present") { *h_min = 1; *h_max = R; return SPSP_OK; }
    if (w == "absent") { *h_min = 0; *h_max = 0; return SPSP_OK; }
    if (w == "all") { *h_min = R; *h_max = R; return SPSP_OK; }
    const size_t eq = w.find('=');
    if (eq != std::string::npos) {
        const std::string name = w.substr(0, eq);
        uint64_t num = 0, den = 1;
        if ((name == "core" || name == "unique" || name == "shell") && fraction(what + eq + 1, &num, &den)) {
            const uint32_t core_min = (uint32_t)((num * R + den - 1) / den);
            if (name == "core") { *h_min = core_min; *h_max = R; }
            else if (name == "unique") { if (core_min > 1) { *h_min = 1; *h_max = 1; } }
            else if (core_min > 2) { *h_min = 2; *h_max = core_min - 1; }
            return SPSP_OK;
        }
    }
    const size_t dots = w.find("..");
    if (dots != std::string::npos && plain(what, what + dots, h_min) && plain(what + dots + 2, what + w.size(), h_max)) return SPSP_OK;
    *h_min = 1; *h_max = 0;
    set_error("'%.60s' is no band of holder counts: union, present, absent, all, core=<t>, unique=<t>, shell=<t> with <t> in (0, 1] and at most six "
              "digits behind the point, or <a>..<b>", what);
    return SPSP_ERR_ARG;
}

// print_containment / print_jaccard (Comparator.cpp:362-460); operator<<(double)
// with setprecision(p) in the default float format is printf's %.*g.
// sortCSV (sort_csv.cpp:26-111): put the rows and columns of a (symmetric, all-vs-all) Jaccard CSV into the order of
// the original file-of-files -- sub_sampler's output list is in OpenMP completion order (SubSampler.cpp:782-786).
// Values pass through a double and are printed with six significant digits, as the reference's `out << double`.
int spsp_sort_csv_host(const char* csv, uint64_t csv_len, const char* fof, uint64_t fof_len, char** text, uint64_t* len) {
    if (!text || !len || (csv_len && !csv) || (fof_len && !fof)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *text = nullptr; *len = 0;
    // fof lines -> rank (first occurrence wins, as std::find does; a final newline yields one empty last name)
    std::unordered_map<std::string, uint32_t> rank_of;
    {
        uint32_t line_no = 0;
        uint64_t a = 0;
        for (uint64_t i = 0; i <= fof_len; ++i) {
            if (i == fof_len || fof[i] == '\n') { rank_of.emplace(std::string(fof + a, i - a), line_no++); a = i + 1; }
        }
    }
    // CSV lines
    std::vector<std::pair<const char*, size_t>> lines;
    for (uint64_t a = 0, i = 0; i <= csv_len; ++i)
        if (i == csv_len || csv[i] == '\n') { lines.emplace_back(csv + a, (size_t)(i - a)); a = i + 1; }
    auto tokens = [](const char* p, size_t n) {   // split() of utils.cpp:609-629: the last field ends at the first non-printable byte
        std::vector<std::string> t;
        size_t a = 0;
        for (size_t i = 0; i < n; ++i) if (p[i] == ',') { t.emplace_back(p + a, i - a); a = i + 1; }
        size_t e = a;
        while (e < n && isprint((unsigned char)p[e])) ++e;
        t.emplace_back(p + a, e - a);
        return t;
    };
    if (lines.empty()) { set_error("empty CSV"); return SPSP_ERR_FORMAT; }
    const std::vector<std::string> head = tokens(lines[0].first, lines[0].second);
    const size_t N = head.size();
    std::vector<std::pair<uint32_t, uint32_t>> order;   // (rank in the fof, column in the input)
    for (size_t c = 0; c < N; ++c) {
        auto it = rank_of.find(head[c]);
        if (it == rank_of.end()) { set_error("column '%s' is not in the file of files", head[c].c_str()); return SPSP_ERR_FORMAT; }
        order.emplace_back(it->second, (uint32_t)c);
    }
    std::sort(order.begin(), order.end());
    for (size_t c = 1; c < N; ++c)
        if (order[c].first == order[c - 1].first) { set_error("column '%s' appears twice", head[order[c].second].c_str()); return SPSP_ERR_FORMAT; }
    std::vector<uint32_t> new_of(N);
    for (size_t r = 0; r < N; ++r) new_of[order[r].second] = (uint32_t)r;
    // Rows.  A matrix of thousands of sketches is nearly all "0" cells (10^8 cells at BASELINE configs[3], 95 000 pairs that
    // share anything): the cells that are not literally "0" are kept as (output row, output column, value) -- the reference
    // fills the TRANSPOSED cell (sort_csv.cpp:83) -- and a row is written as runs of "0," between them.  Lines are independent:
    // parsed and printed by a few threads (the round-3 form built 10^8 std::strings and an N x N array of doubles: 8 s at
    // N = 6 000 on one thread).
    size_t n_rows = 0;                                   // consecutive lines that can hold a row (sort_csv.cpp:80 stops at the first that cannot)
    while (1 + n_rows < lines.size() && lines[1 + n_rows].second >= N) ++n_rows;
    const size_t parse_rows = n_rows < N ? n_rows : N;
    struct Cell { uint32_t orow, ocol; double x; };
    unsigned workers = std::thread::hardware_concurrency();
    if (workers == 0) workers = 1;
    if (workers > 16) workers = 16;
    if (N * N < (1u << 20)) workers = 1;
    if (workers > parse_rows) workers = parse_rows ? (unsigned)parse_rows : 1;
    std::vector<std::vector<Cell>> found(workers);
    std::vector<size_t> bad_row(workers, (size_t)-1);       // first row this worker could not parse
    std::vector<std::string> bad_msg(workers);
    auto parse = [&](unsigned w) {
        char buf[64];
        for (size_t r = w; r < parse_rows; r += workers) {
            const char* p = lines[1 + r].first;
            const size_t n = lines[1 + r].second;
            size_t a = 0, c = 0;
            bool failed = false;
            auto cell = [&](size_t b) {                  // cell c = [a, b)
                const size_t l = b - a;
                if (l == 1 && p[a] == '0') return;       // the common case: 0 -> "0"
                if (l == 0 || l >= sizeof buf) { failed = true; return; }
                memcpy(buf, p + a, l); buf[l] = 0;
                char* endp = nullptr;
                const double x = strtod(buf, &endp);
                if (endp == buf) { failed = true; return; }
                found[w].push_back(Cell{new_of[c], new_of[r], x});
            };
            for (size_t i = 0; i < n && c < N && !failed; ++i)
                if (p[i] == ',') { cell(i); if (failed) { char t[96]; snprintf(t, sizeof t, "row %zu, column %zu: not a number", r, c); bad_msg[w] = t; } a = i + 1; ++c; }
            if (!failed && c < N) {                       // the last field ends at the first non-printable byte (split(), utils.cpp:609-629)
                size_t e = a;
                while (e < n && isprint((unsigned char)p[e])) ++e;
                if (c + 1 < N) { char t[96]; snprintf(t, sizeof t, "row %zu has %zu values, expected %zu", r, c + 1, N); bad_msg[w] = t; failed = true; }
                else { cell(e); if (failed) { char t[96]; snprintf(t, sizeof t, "row %zu, column %zu: not a number", r, c); bad_msg[w] = t; } ++c; }
            }
            if (failed) { bad_row[w] = r; return; }
        }
    };
    {
        std::vector<std::thread> pool;
        for (unsigned w = 1; w < workers; ++w) pool.emplace_back(parse, w);
        parse(0);
        for (auto& th : pool) th.join();
    }
    {
        unsigned first = workers;
        for (unsigned w = 0; w < workers; ++w) if (bad_row[w] != (size_t)-1 && (first == workers || bad_row[w] < bad_row[first])) first = w;
        if (first != workers) { set_error("%s", bad_msg[first].c_str()); return SPSP_ERR_FORMAT; }
    }
    if (n_rows > N) { set_error("more than %zu rows", N); return SPSP_ERR_FORMAT; }
    if (n_rows != N) { set_error("%zu rows for %zu columns (a containment file, or a query-mode matrix?)", n_rows, N); return SPSP_ERR_FORMAT; }
    // cells by output row, then by column
    std::vector<size_t> at(N + 1, 0);
    for (auto& v : found) for (const Cell& c : v) ++at[c.orow + 1];
    for (size_t i = 0; i < N; ++i) at[i + 1] += at[i];
    std::vector<std::pair<uint32_t, double>> adj(at[N]);
    {
        std::vector<size_t> cur(at.begin(), at.end() - 1);
        for (auto& v : found) for (const Cell& c : v) adj[cur[c.orow]++] = std::make_pair(c.ocol, c.x);
    }
    std::vector<std::vector<Cell>>().swap(found);
    for (size_t i = 0; i < N; ++i) {                      // the diagonal must be 1 (the reference stops at the first that is not, sort_csv.cpp:100-104)
        double d = 0;
        for (size_t e = at[i]; e < at[i + 1]; ++e) if (adj[e].first == i) d = adj[e].second;
        if (d != 1) { set_error("diagonal entry %zu is not 1 (the reference stops here)", i); return SPSP_ERR_FORMAT; }
    }
    std::string head_out;
    for (size_t r = 0; r < N; ++r) { head_out += head[order[r].second]; head_out += (r + 1 != N) ? ',' : '\n'; }
    static const std::string zero_run = []() { std::string z; z.reserve(8192); for (int i = 0; i < 4096; ++i) z += "0,"; return z; }();
    std::vector<std::string> parts(workers);
    auto print = [&](unsigned w) {
        std::string& out = parts[w];
        const size_t r0 = N * w / workers, r1 = N * (w + 1) / workers;
        out.reserve((r1 - r0) * N * 2 + 4096);
        char num[40];
        for (size_t i = r0; i < r1; ++i) {
            std::sort(adj.begin() + at[i], adj.begin() + at[i + 1], [](const std::pair<uint32_t, double>& x, const std::pair<uint32_t, double>& y) { return x.first < y.first; });
            size_t col = 0;
            auto zeros_to = [&](size_t upto) {
                size_t z = upto - col;
                while (z) { const size_t take = z < 4096 ? z : 4096; out.append(zero_run.data(), take * 2); z -= take; }
                col = upto;
            };
            for (size_t e = at[i]; e < at[i + 1]; ++e) {
                if (e + 1 < at[i + 1] && adj[e + 1].first == adj[e].first) continue;      // (a column given twice cannot happen: columns are a permutation)
                zeros_to(adj[e].first);
                out.append(num, (size_t)snprintf(num, sizeof num, "%g", adj[e].second));
                out += ',';
                col = adj[e].first + 1;
            }
            zeros_to(N);
            out.back() = '\n';
        }
    };
    {
        std::vector<std::thread> pool;
        for (unsigned w = 1; w < workers; ++w) pool.emplace_back(print, w);
        print(0);
        for (auto& th : pool) th.join();
    }
    size_t total = head_out.size();
    for (auto& p2 : parts) total += p2.size();
    char* buf = (char*)malloc(total + 1);
    if (!buf) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    size_t pos = 0;
    memcpy(buf, head_out.data(), head_out.size()); pos += head_out.size();
    for (auto& p2 : parts) { memcpy(buf + pos, p2.data(), p2.size()); pos += p2.size(); }
    buf[total] = 0;
    *text = buf; *len = total;
    return SPSP_OK;
}

// mirrored: cell (i, j) is also stored at (j, i) -- a row is then read left to right instead of down a column for j < i
// (10^4 sketches: 5 x 10^7 reads 40 KB apart per matrix otherwise)
// printf's %.*g (what `out << setprecision(p) << double` prints, Comparator.cpp:362-460) by std::to_chars: the same characters by
// the standard's word (general format with a precision = "as if by printf %.*g in the C locale"; 15 x 10^6 random scores at five
// precisions compared equal) at a third of the time -- a 10^8-cell matrix of 10^4 sketches is 2 x 10^5 numbers per matrix
static inline int format_g(char* buf, size_t cap, int precision, double v) {
    if (precision >= 0) {
        const std::to_chars_result r = std::to_chars(buf, buf + cap, v, std::chars_format::general, precision);
        if (r.ec == std::errc()) return (int)(r.ptr - buf);
    }
    return snprintf(buf, cap, "%.*g", precision, v);
}
static int csv_impl(int jaccard, const char* const* names, uint32_t n, uint32_t n_query, const uint32_t* inter,
                    const uint64_t* card, int precision, double min_threshold, char** text, uint64_t* len, bool mirrored) {
    if (!text || !len || (n && (!names || !inter || !card))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::string head;
    for (uint32_t i = 0; i < n; ++i) { head += names[i]; head += (i + 1 != n) ? ',' : '\n'; }
    if (!jaccard) head += '\n';
    // rows are independent: formatted by a few host threads (row blocks), concatenated in order ("next" row N3)
    const uint32_t rows = n < n_query ? n : n_query;
    // a matrix of thousands of sketches is nearly all zeros (species that share no k-mer): runs of "0," are copied from a
    // constant instead of being appended cell by cell
    static const std::string zero_run = []() { std::string z; z.reserve(8192); for (int i = 0; i < 4096; ++i) z += "0,"; return z; }();
    auto format_rows = [&](uint32_t r0, uint32_t r1, std::string& out) {
        char num[64];
        out.reserve((size_t)(r1 - r0) * n * 2 + 4096);
        for (uint32_t i = r0; i < r1; ++i) {
            const uint32_t* row = inter + (uint64_t)i * n;
            uint32_t zeros = 0;                                   // cells "0," not written yet
            auto flush = [&]() { while (zeros) { const uint32_t take = zeros < 4096 ? zeros : 4096; out.append(zero_run.data(), (size_t)take * 2); zeros -= take; } };
            for (uint32_t j = 0; j < n; ++j) {
                uint32_t sc = 0;
                if (i != j) sc = (mirrored || i < j) ? row[j] : inter[(uint64_t)j * n + i];
                if (i != j && sc == 0) { ++zeros; continue; }
                flush();
                if (i == j) out += '1';
                else {
                    const double score = jaccard ? (double)sc / (double)(card[i] + card[j] - sc) : (double)sc / (double)card[i];
                    if (score < min_threshold) out += '0';
                    else { const int l = format_g(num, sizeof num, precision, score); out.append(num, l); }
                }
                out += ',';
            }
            flush();
            out.back() = '\n';                                    // (the row's last separator)
        }
    };
    unsigned workers = std::thread::hardware_concurrency();
    if (workers == 0) workers = 1;
    if (workers > 16) workers = 16;
    if ((uint64_t)rows * n < (1u << 18)) workers = 1;          // small matrices: not worth a thread
    if (workers > rows) workers = rows ? rows : 1;
    std::vector<std::string> parts(workers);
    {
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < workers; ++w) {
            const uint32_t r0 = (uint32_t)((uint64_t)rows * w / workers), r1 = (uint32_t)((uint64_t)rows * (w + 1) / workers);
            if (w + 1 == workers) format_rows(r0, r1, parts[w]);
            else pool.emplace_back(format_rows, r0, r1, std::ref(parts[w]));
        }
        for (auto& th : pool) th.join();
    }
    size_t total = head.size();
    for (auto& p2 : parts) total += p2.size();
    *text = (char*)malloc(total + 1);
    if (!*text) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    size_t at = 0;
    memcpy(*text, head.data(), head.size()); at += head.size();
    for (auto& p2 : parts) { memcpy(*text + at, p2.data(), p2.size()); at += p2.size(); }
    (*text)[total] = 0;
    *len = total;
    return SPSP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Rows of a sparse pair matrix straight into a gzip member (round 5).  A row of a 10^4-sketch matrix is ~12 runs of "0,"
// between ~10 numbers; formatted as text and handed to zlib it is 20 KB through deflate's match finder and crc32 -- 42 ms of
// thread time per 10^8-cell matrix.  Here the row never exists as text: a run of z cells is the two literals "0," and
// ceil((2z - 2) / 258) matches of distance 2 in ONE fixed-Huffman deflate block (RFC 1951 3.2.6), and the member's CRC-32
// takes the run as 16 table steps -- crc(A || B) = crc(A) * x^(8 |B|) + crc(B) over GF(2), with the operators x^(16 * 2^t)
// (2^t cells) as byte tables and crc("0," x 2^t) precomputed.  gunzip gives the bytes the text path writes (the tests read
// every member back through zlib, which checks CRC-32 and ISIZE).
namespace {
struct ZeroRunCrc {
    uint32_t tab[17][4][256];                 // tab[t]: multiplication of a (reflected) CRC value by x^(16 * 2^t), byte-wise
    uint32_t crc[17];                         // crc32 of "0," x 2^t
    static uint32_t times(const uint32_t* mat, uint32_t vec) { uint32_t s = 0; for (int i = 0; vec; vec >>= 1, ++i) if (vec & 1u) s ^= mat[i]; return s; }
    ZeroRunCrc() {
        uint32_t a[32], b[32];
        a[0] = 0xedb88320u;                    // the operator of ONE zero bit (zlib crc32_combine): the polynomial, then the shifts
        for (int n = 1; n < 32; ++n) a[n] = 1u << (n - 1);
        auto square = [](uint32_t* dst, const uint32_t* src) { for (int n = 0; n < 32; ++n) dst[n] = times(src, src[n]); };
        square(b, a); square(a, b); square(b, a); square(a, b);   // 2, 4, 8, 16 bits: a = two zero bytes = one cell
        const char cell[2] = {'0', ','};
        for (int t = 0; t <= 16; ++t) {
            for (int by = 0; by < 4; ++by)
                for (uint32_t v = 0; v < 256; ++v) tab[t][by][v] = times(a, v << (8 * by));
            if (t == 0) crc[0] = (uint32_t)crc32(0L, (const Bytef*)cell, 2);
            else crc[t] = mul(t - 1, crc[t - 1]) ^ crc[t - 1];   // 2^t cells = 2^(t-1) cells followed by 2^(t-1) cells
            square(b, a); memcpy(a, b, sizeof a);
        }
    }
    uint32_t mul(int t, uint32_t c) const { return tab[t][0][c & 255u] ^ tab[t][1][(c >> 8) & 255u] ^ tab[t][2][(c >> 16) & 255u] ^ tab[t][3][c >> 24]; }
    uint32_t append(uint32_t c, uint32_t cells) const {            // crc of (what c covers) followed by `cells` x "0,"
        for (int t = 0; cells; cells >>= 1, ++t) if (cells & 1u) c = mul(t, c) ^ crc[t];
        return c;
    }
};
static const ZeroRunCrc& zero_run_crc() { static const ZeroRunCrc z; return z; }

struct StringSink {
    std::string* out;
    void bytes(const char* p, size_t n) { out->append(p, n); }
    void zeros(uint32_t cells) {
        static const std::string run = []() { std::string z; z.reserve(8192); for (int i = 0; i < 4096; ++i) z += "0,"; return z; }();
        while (cells) { const uint32_t take = cells < 4096 ? cells : 4096; out->append(run.data(), (size_t)take * 2); cells -= take; }
    }
};
struct GzSink {                                // one gzip member: header, ONE fixed-Huffman block, CRC-32, ISIZE
    std::vector<uint8_t>* out;
    uint64_t acc = 0; int nbits = 0;
    uint32_t crc = 0; uint64_t isize = 0;
    static uint32_t rev(uint32_t v, int n) { uint32_t r = 0; for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i); return r; }
    // the bit patterns of the fixed code, made once: a literal's (8 or 9 bits), and the match of 258 bytes at distance 2 (13 bits)
    struct Codes {
        uint16_t lit[256]; uint8_t lit_len[256]; uint32_t m258; int m258_len;
        Codes() {
            for (uint32_t b = 0; b < 256; ++b) { if (b < 144) { lit[b] = (uint16_t)rev(0x30u + b, 8); lit_len[b] = 8; } else { lit[b] = (uint16_t)rev(0x190u + (b - 144u), 9); lit_len[b] = 9; } }
            m258 = rev(0xc0u + 5u, 8) | (rev(1u, 5) << 8); m258_len = 13;      // symbol 285 (no extra bits), distance code 1
        }
    };
    static const Codes& codes() { static const Codes c; return c; }
    void put(uint32_t v, int n) {               // n bits, least significant first (n <= 32, at most 7 bits pending: 39 fit)
        acc |= (uint64_t)v << nbits; nbits += n;
        if (nbits >= 32) {                      // four bytes at a time
            const size_t at = out->size();
            out->resize(at + 4);
            const uint32_t w = (uint32_t)acc;
            memcpy(out->data() + at, &w, 4);
            acc >>= 32; nbits -= 32;
        }
    }
    void flush_bytes() { while (nbits >= 8) { out->push_back((uint8_t)acc); acc >>= 8; nbits -= 8; } }
    void begin() {
        static const uint8_t hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
        out->insert(out->end(), hdr, hdr + 10);
        put(1, 1); put(1, 2);                   // BFINAL = 1, BTYPE = 01
    }
    void literal(uint8_t b) { const Codes& C = codes(); put(C.lit[b], C.lit_len[b]); }
    void match2(uint32_t len) {                 // `len` bytes (3 .. 258) copied from distance 2
        if (len == 258) { const Codes& C = codes(); put(C.m258, C.m258_len); return; }
        static const uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const uint8_t extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        int c = 28;
        while (base[c] > len) --c;              // (258 has a code of its own; 227 .. 257 are code 284 + extra bits)
        const uint32_t sym = 257u + (uint32_t)c;
        if (sym < 280) put(rev(sym - 256u, 7), 7); else put(rev(0xc0u + (sym - 280u), 8), 8);
        if (extra[c]) put(len - base[c], extra[c]);
        put(rev(1u, 5), 5);                     // distance code 1 = distance 2, no extra bits
    }
    void bytes(const char* p, size_t n) {
        for (size_t i = 0; i < n; ++i) literal((uint8_t)p[i]);
        crc = (uint32_t)crc32(crc, (const Bytef*)p, (uInt)n); isize += n;
    }
    void zeros(uint32_t cells) {
        if (!cells) return;
        literal('0'); literal(',');
        uint64_t rem = 2ull * cells - 2;
        while (rem >= 258) { match2(258); rem -= 258; }
        if (rem >= 4) match2((uint32_t)rem); else if (rem == 2) { literal('0'); literal(','); }
        crc = zero_run_crc().append(crc, cells); isize += 2ull * cells;
    }
    void end() {
        put(0, 7);                              // end of block (symbol 256: seven zero bits)
        flush_bytes();
        if (nbits) { put(0, 8 - nbits); flush_bytes(); }
        for (int i = 0; i < 4; ++i) out->push_back((uint8_t)(crc >> (8 * i)));
        for (int i = 0; i < 4; ++i) out->push_back((uint8_t)((uint32_t)isize >> (8 * i)));
    }
};
}  // namespace

// The same bytes from the SPARSE form of the pair matrix (packed cells i << 48 | j << 32 | count, i < j, every pair at most
// once): a comparison of thousands of sketches returns ~10 non-zero partners per row, and a row is then "0," runs between
// them -- no n x n matrix is built or scanned (10^4 sketches: 2 x 400 MB of reads per matrix before).
static int deflate_member(const uint8_t* data, uint64_t len, int level, std::vector<uint8_t>& out);
// gz_path != nullptr: nothing is returned as text; row blocks of ~8 MB are formatted AND deflated by the workers, one gzip
// member each, and written in order (a valid gzip file that zstr / zlib / gunzip read back as one stream, like the members
// of spsp_write_gz_host): the 200 MB of a 10^8-cell matrix never exist in one piece.  times[0] / times[1]: the workers'
// formatting / deflate + write seconds, summed and divided by the worker count.
static int csv_cells_impl(int jaccard, const char* const* names, uint32_t n, uint32_t n_query, const std::vector<uint64_t>& cells,
                          const uint64_t* card, int precision, double min_threshold, char** text, uint64_t* len,
                          const char* gz_path = nullptr, int gz_level = 1, double* times = nullptr) {
    std::string head;
    for (uint32_t i = 0; i < n; ++i) { head += names[i]; head += (i + 1 != n) ? ',' : '\n'; }
    if (!jaccard) head += '\n';
    const uint32_t rows = n < n_query ? n : n_query;
    // partners of every printed row, by column
    std::vector<uint32_t> deg((size_t)rows + 1, 0);
    for (uint64_t c : cells) {
        const uint32_t i = (uint32_t)(c >> 48), j = (uint32_t)(c >> 32) & 0xffffu;
        if (i < rows) ++deg[i + 1];
        if (j < rows) ++deg[j + 1];
    }
    for (uint32_t i = 0; i < rows; ++i) deg[i + 1] += deg[i];
    std::vector<uint64_t> adj((size_t)deg[rows]);                  // partner << 32 | count
    {
        std::vector<uint32_t> at(deg.begin(), deg.end() - 1);
        for (uint64_t c : cells) {
            const uint32_t i = (uint32_t)(c >> 48), j = (uint32_t)(c >> 32) & 0xffffu;
            if (i < rows) adj[at[i]++] = ((uint64_t)j << 32) | (uint32_t)c;
            if (j < rows) adj[at[j]++] = ((uint64_t)i << 32) | (uint32_t)c;
        }
    }
    // rows [r0, r1) into a sink: text (StringSink) or a gzip member made directly (GzSink).  A cell is its text and ',' -- '\n'
    // for the row's last cell; a run of zeros that reaches the end of the row is one cell shorter and ends in "0\n"
    auto format_rows = [&](uint32_t r0, uint32_t r1, auto& sink) {
        char num[64];
        for (uint32_t i = r0; i < r1; ++i) {
            std::sort(adj.begin() + deg[i], adj.begin() + deg[i + 1]);
            uint32_t col = 0;
            auto zeros_to = [&](uint32_t upto) {                 // cells [col, upto) are "0,"
                if (upto > col) {
                    if (upto == n) { sink.zeros(upto - col - 1); sink.bytes("0\n", 2); }
                    else sink.zeros(upto - col);
                }
                col = upto;
            };
            auto cell = [&](const char* p, size_t l, uint32_t at) {   // the cell of column `at`: its text and the separator in one piece
                char piece[72];
                memcpy(piece, p, l);
                piece[l] = at + 1 == n ? '\n' : ',';
                sink.bytes(piece, l + 1);
                col = at + 1;
            };
            bool diag_done = false;
            auto diagonal = [&]() { zeros_to(i); cell("1", 1, i); diag_done = true; };
            for (uint32_t e = deg[i]; e < deg[i + 1]; ++e) {
                const uint32_t j = (uint32_t)(adj[e] >> 32), sc = (uint32_t)adj[e];
                if (!diag_done && j > i) diagonal();
                zeros_to(j);
                const double score = jaccard ? (double)sc / (double)(card[i] + card[j] - sc) : (double)sc / (double)card[i];
                if (score < min_threshold) cell("0", 1, j);
                else { const int l = format_g(num, sizeof num, precision, score); cell(num, (size_t)l, j); }
            }
            if (!diag_done) diagonal();
            zeros_to(n);
        }
    };
    unsigned workers = std::thread::hardware_concurrency();
    if (workers == 0) workers = 1;
    if (workers > 16) workers = 16;
    if (workers > rows) workers = rows ? rows : 1;
    if (gz_path) {
        // rows per block: ~8 MB of text when the rows are mostly "0," -- and never fewer than four blocks per worker: a DENSE matrix
        // (one species: every cell a 9-byte number) of 1 200 rows was ONE block, formatted and deflated by one thread, 0.46 of a 0.48 s call
        uint32_t rpb = std::max<uint32_t>(1, (uint32_t)((8ull << 20) / (2ull * (n ? n : 1))));
        rpb = std::max<uint32_t>(1, std::min<uint32_t>(rpb, rows / (4 * workers)));
        const uint32_t n_blocks = rows ? (rows + rpb - 1) / rpb : 0;
        std::vector<std::vector<uint8_t>> gz((size_t)n_blocks + 1);
        std::vector<int> rcs((size_t)n_blocks + 1, SPSP_OK);
        std::atomic<uint32_t> next(0);
        std::vector<double> t_fmt(workers, 0.0), t_gz(workers, 0.0);
        rcs[0] = deflate_member((const uint8_t*)head.data(), head.size(), gz_level, gz[0]);        // the header line(s): a member of their own
        auto work = [&](unsigned w) {
            for (;;) {
                const uint32_t b = next.fetch_add(1);
                if (b >= n_blocks) break;
                const double t0 = now_s();
                GzSink sink{&gz[b + 1]};                          // formatted and deflated in one go: the rows never exist as text
                sink.begin();
                format_rows(b * rpb, std::min(rows, (b + 1) * rpb), sink);
                sink.end();
                t_fmt[w] += now_s() - t0;
            }
        };
        if (workers > n_blocks) workers = n_blocks ? n_blocks : 1;
        {
            std::vector<std::thread> pool;
            for (unsigned w = 1; w < workers; ++w) pool.emplace_back(work, w);
            work(0);
            for (auto& th : pool) th.join();
        }
        const double t2 = now_s();
        for (int r : rcs) if (r) { set_error("deflate failed"); return r; }
        FILE* f = fopen(gz_path, "wb");
        if (!f) { set_error("cannot create '%s'", gz_path); return SPSP_ERR_IO; }
        int rc = SPSP_OK;
        for (auto& m : gz) if (!rc && fwrite(m.data(), 1, m.size(), f) != m.size()) { set_error("short write to '%s'", gz_path); rc = SPSP_ERR_IO; }
        if (fclose(f) != 0 && !rc) { set_error("close failed for '%s'", gz_path); rc = SPSP_ERR_IO; }
        if (times) {
            double a = 0, b2 = 0;
            for (unsigned w = 0; w < workers; ++w) { a += t_fmt[w]; b2 += t_gz[w]; }
            times[0] = a / workers; times[1] = b2 / workers + (now_s() - t2);
        }
        return rc;
    }
    std::vector<std::string> parts(workers);
    {
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < workers; ++w) {
            const uint32_t r0 = (uint32_t)((uint64_t)rows * w / workers), r1 = (uint32_t)((uint64_t)rows * (w + 1) / workers);
            auto job = [&format_rows, &parts, n](uint32_t a, uint32_t z, unsigned which) {
                parts[which].reserve((size_t)(z - a) * n * 2 + 4096);
                StringSink sink{&parts[which]};
                format_rows(a, z, sink);
            };
            if (w + 1 == workers) job(r0, r1, w);
            else pool.emplace_back(job, r0, r1, w);
        }
        for (auto& th : pool) th.join();
    }
    size_t total = head.size();
    for (auto& p2 : parts) total += p2.size();
    *text = (char*)malloc(total + 1);
    if (!*text) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    size_t at = 0;
    memcpy(*text, head.data(), head.size()); at += head.size();
    for (auto& p2 : parts) { memcpy(*text + at, p2.data(), p2.size()); at += p2.size(); }
    (*text)[total] = 0;
    *len = total;
    return SPSP_OK;
}

int spsp_csv_cells_host(int jaccard, const char* const* names, uint32_t n, uint32_t n_query, const uint64_t* cells, uint64_t n_cells,
                        const uint64_t* card, int precision, double min_threshold, char** text, uint64_t* len) {
    if (!text || !len || (n && (!names || !card)) || (n_cells && !cells)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n > 65535) { set_error("at most 65535 sketches (a packed cell holds two 16-bit sketch numbers)"); return SPSP_ERR_ARG; }
    std::vector<uint64_t> v(cells, cells + n_cells);
    std::sort(v.begin(), v.end());
    for (size_t e = 0; e < v.size(); ++e) {
        const uint32_t i = (uint32_t)(v[e] >> 48), j = (uint32_t)(v[e] >> 32) & 0xffffu;
        if (i >= j || j >= n) { set_error("cell %zu names the pair (%u, %u): not i < j < n", e, i, j); return SPSP_ERR_FORMAT; }
        if (e && (v[e] >> 32) == (v[e - 1] >> 32)) { set_error("the pair (%u, %u) occurs twice: add partial cells up first (spsp_matrix_add_cells_device)", i, j); return SPSP_ERR_FORMAT; }
    }
    return csv_cells_impl(jaccard, names, n, n_query, v, card, precision, min_threshold, text, len);
}

int spsp_csv_cells_gz_host(int jaccard, const char* const* names, uint32_t n, uint32_t n_query, const uint64_t* cells, uint64_t n_cells,
                           const uint64_t* card, int precision, double min_threshold, const char* gz_path) {
    if (!gz_path || (n && (!names || !card)) || (n_cells && !cells)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n > 65535) { set_error("at most 65535 sketches (a packed cell holds two 16-bit sketch numbers)"); return SPSP_ERR_ARG; }
    std::vector<uint64_t> v(cells, cells + n_cells);
    std::sort(v.begin(), v.end());
    for (size_t e = 0; e < v.size(); ++e) {
        const uint32_t i = (uint32_t)(v[e] >> 48), j = (uint32_t)(v[e] >> 32) & 0xffffu;
        if (i >= j || j >= n) { set_error("cell %zu names the pair (%u, %u): not i < j < n", e, i, j); return SPSP_ERR_FORMAT; }
        if (e && (v[e] >> 32) == (v[e - 1] >> 32)) { set_error("the pair (%u, %u) occurs twice: add partial cells up first (spsp_matrix_add_cells_device)", i, j); return SPSP_ERR_FORMAT; }
    }
    return csv_cells_impl(jaccard, names, n, n_query, v, card, precision, min_threshold, nullptr, nullptr, gz_path, 1, nullptr);
}

int spsp_csv_host(int jaccard, const char* const* names, uint32_t n, uint32_t n_query, const uint32_t* inter,
                  const uint64_t* card, int precision, double min_threshold, char** text, uint64_t* len) {
    return csv_impl(jaccard, names, n, n_query, inter, card, precision, min_threshold, text, len, false);
}

// Three system calls for a small file (open, one read that comes back short, close): where system calls are the cost -- 10^4
// sketch files of 3 KB, on hosts that serialise them -- fopen + fstat + two freads + fclose were twice that.
static int slurp(const char* path, uint8_t** raw, uint64_t* n) {
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) { set_error("cannot open '%s'", path); return SPSP_ERR_IO; }
    // the first 64 KiB land in a buffer the thread keeps (a fresh 64 KiB block per file had malloc trimming the heap per file)
    struct Scratch { uint8_t* p = (uint8_t*)malloc((1u << 16) + 64); ~Scratch() { free(p); } };
    static thread_local Scratch scratch;
    size_t cap = 1u << 16;
    uint8_t* buf = scratch.p;
    bool own = false;
    size_t got = 0;
    bool regular_known = false, regular = false;
    while (buf) {
        const ssize_t r = read(fd, buf + got, cap - got);
        if (r < 0) { if (errno == EINTR) continue; if (own) free(buf); close(fd); set_error("cannot read '%s'", path); return SPSP_ERR_IO; }
        if (r == 0) break;
        got += (size_t)r;
        if (got < cap) {
            // a short read ends a REGULAR file (pipes and ttys may come back short at any time)
            if (!regular_known) { struct stat st; regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && (size_t)st.st_size == got; regular_known = true; if (regular) break; }
            continue;
        }
        if (!regular_known) {   // a big file: size the buffer once instead of doubling through it
            struct stat st;
            regular_known = true;
            if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && (size_t)st.st_size > cap) cap = (size_t)st.st_size + 1; else cap *= 2;
        } else cap *= 2;
        uint8_t* nb = own ? (uint8_t*)realloc(buf, cap + 64) : (uint8_t*)malloc(cap + 64);
        if (nb && !own) memcpy(nb, buf, got);
        if (!nb) { if (own) free(buf); buf = nullptr; } else buf = nb;
        own = true;
    }
    close(fd);
    if (buf && !own) {   // small file: an exact-size copy out of the scratch
        uint8_t* nb = (uint8_t*)malloc(got + 64);
        if (nb) memcpy(nb, buf, got);
        buf = nb;
    }
    if (!buf) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    *raw = buf; *n = got;
    return SPSP_OK;
}

int spsp_read_file_host(const char* path, uint8_t** data, uint64_t* len) {
    if (!path || !data || !len) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    uint8_t* raw = nullptr; uint64_t n = 0;
    int rc = slurp(path, &raw, &n);
    if (rc) return rc;
    const bool packed = n >= 2 && ((raw[0] == 0x1F && raw[1] == 0x8B) ||
                                   (raw[0] == 0x78 && (raw[1] == 0x01 || raw[1] == 0x9C || raw[1] == 0xDA)));
    if (!packed) { *data = raw; *len = n; return SPSP_OK; }   // plain text passes through (zstr autodetect)
    std::vector<uint8_t> plain;
    rc = inflate_all(raw, n, plain);
    free(raw);
    if (rc) return rc;
    *data = (uint8_t*)malloc(plain.size() + 64);
    if (!*data) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    if (!plain.empty()) memcpy(*data, plain.data(), plain.size());
    *len = plain.size();
    return SPSP_OK;
}

// zstr::ofstream(filename, expbuffer, level) -> gzip container (zstr.hpp:78-82)
static int deflate_member(const uint8_t* data, uint64_t len, int level, std::vector<uint8_t>& out) {
    // one deflator per thread and level, reset per member (deflateInit2 is 268 KB of allocation per call: per sketch, in the
    // file pipeline)
    struct Deflator { z_stream zs; int level = -100; ~Deflator() { if (level != -100) deflateEnd(&zs); } };
    static thread_local Deflator D;
    if (D.level != level) {
        if (D.level != -100) { deflateEnd(&D.zs); D.level = -100; }
        memset(&D.zs, 0, sizeof D.zs);
        if (deflateInit2(&D.zs, level, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return SPSP_ERR_IO;
        D.level = level;
    } else if (deflateReset(&D.zs) != Z_OK) return SPSP_ERR_IO;
    z_stream& zs = D.zs;
    out.resize(deflateBound(&zs, (uLong)len) + 64);
    zs.next_in = const_cast<Bytef*>(data);
    zs.avail_in = (uInt)len;
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    const int ret = deflate(&zs, Z_FINISH);
    const size_t have = out.size() - zs.avail_out;
    if (ret != Z_STREAM_END) return SPSP_ERR_IO;
    out.resize(have);
    return SPSP_OK;
}

int spsp_write_gz_host(const char* path, const uint8_t* data, uint64_t len, int level) {
    if (!path || (len && !data)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    // plain descriptors, not stdio: fopen/fclose take a process-wide lock (the list of open FILEs), and the file pipeline
    // writes one sketch per task on every host thread
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) { set_error("cannot create '%s'", path); return SPSP_ERR_IO; }
    auto write_all = [&](const uint8_t* p, size_t n) {
        while (n) {
            const ssize_t w = write(fd, p, n);
            if (w < 0) { if (errno == EINTR) continue; return false; }
            p += w; n -= (size_t)w;
        }
        return true;
    };
    // One gzip member per 16 MiB of payload.  Small outputs (every sketch) are a single member, exactly what
    // zstr::ofstream writes; large CSVs are compressed member by member on a few threads -- a valid gzip file
    // that zstr / zlib / gunzip read back as one stream (zstr.hpp:198-203 restarts the inflator per member).
    // (beyond 16 MiB the members shrink to 1 MiB at the least, so that the 28 MB sketch of a 4 Gbp record set at -s 100 keeps
    // every worker busy: 0.43 s with 16 MiB members, 0.11 s with 4 MiB -- seven members on sixteen threads)
    unsigned workers = std::thread::hardware_concurrency();
    if (workers == 0) workers = 1;
    if (workers > 16) workers = 16;
    uint64_t chunk = 16ull << 20;
    if (len > chunk) chunk = std::max<uint64_t>(1ull << 20, std::min<uint64_t>(chunk, ((len + workers - 1) / workers + 0xfffffull) & ~0xfffffull));
    const uint64_t n_chunks = len ? (len + chunk - 1) / chunk : 1;
    if (workers > n_chunks) workers = (unsigned)n_chunks;
    int rc = SPSP_OK;
    for (uint64_t c0 = 0; c0 < n_chunks && !rc; c0 += workers) {
        const unsigned batch = (unsigned)std::min<uint64_t>(workers, n_chunks - c0);
        std::vector<std::vector<uint8_t>> outs(batch);
        std::vector<int> rcs(batch, SPSP_OK);
        std::vector<std::thread> pool;
        auto job = [&](unsigned b) {
            const uint64_t off = (c0 + b) * chunk;
            const uint64_t take = len > off ? std::min<uint64_t>(chunk, len - off) : 0;
            rcs[b] = deflate_member(data + off, take, level, outs[b]);
        };
        for (unsigned b = 1; b < batch; ++b) pool.emplace_back(job, b);
        job(0);
        for (auto& th : pool) th.join();
        for (unsigned b = 0; b < batch && !rc; ++b) {
            if (rcs[b]) { set_error("deflate failed"); rc = rcs[b]; break; }
            if (!write_all(outs[b].data(), outs[b].size())) { set_error("short write to '%s'", path); rc = SPSP_ERR_IO; }
        }
    }
    if (close(fd) != 0 && !rc) { set_error("close failed for '%s'", path); rc = SPSP_ERR_IO; }
    return rc;
}

int spsp_stage_times_read(spsp_ctx* ctx, spsp_stage_times* out, int reset) {
    if (!ctx || !out) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *out = ctx->stages;
    if (reset) ctx->stages = spsp_stage_times{};
    return SPSP_OK;
}

}  // extern "C"

namespace spsp {
void LoadedSketches::release() {
    for (size_t i = 0; i < data.size(); ++i) { if (own[i]) free(data[i]); data[i] = nullptr; }
}

int load_sketch_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, double rate, LoadedSketches* L) {
    const double t0 = L->t0 = now_s();
    if (rate != SPSP_RATE_AS_IS && rate != SPSP_RATE_COARSEST && !(rate > 0)) { set_error("sampling rate %g: must be positive", rate); return SPSP_ERR_ARG; }
    ctx->stages.compare_calls += 1;
    L->data.assign(n, nullptr); L->len.assign(n, 0); L->own.assign(n, 1);
    std::vector<uint8_t*>& datas = L->data;
    std::vector<uint64_t>& lens = L->len;
    std::vector<uint8_t>& own = L->own;
    std::vector<int> rcs(n, SPSP_OK);
    std::vector<std::string> errs(n);
    // Many sketch files: every reader thread takes a RANGE of the files and lays their payloads down back to back (each at the
    // 16-byte-rounded end of the one before) in a region of its own that the context keeps; the decoder finds payloads that lie
    // as it would lay them out and uploads them from where they are, a copy per region (spsp_decode.hip).  One pass: open / read /
    // close do not scale with threads on the hosts measured (10 000 files: 13 ms from one thread and from sixteen,
    // tools/exp/open_scaling.sh), the inflating does -- so a file is inflated by the thread that read it while the others wait for
    // the kernel (two passes, all reads then all inflates into one block by the trailers' lengths, were 13 + 12 ms).
    // datas[i] then points INTO a region (own[i] == 0).
    unsigned workers = std::thread::hardware_concurrency();
    if (workers == 0) workers = 1;
    if (workers > 16) workers = 16;
    if (workers > n) workers = n ? n : 1;
    auto on_threads = [&](const std::function<void(uint32_t)>& one) {
        std::atomic<uint32_t> next(0);
        auto work = [&]() { for (;;) { const uint32_t i = next.fetch_add(1); if (i >= n) break; one(i); } };
        std::vector<std::thread> pool;
        for (unsigned w = 1; w < workers; ++w) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
    };
    // One file at a time per worker: no N open streams (Comparator.cpp:45-50).  Decoding (strDecompressor, inject_minimizer, the
    // k-mer walks, sort, unique) happens for all sketches at once on the GPU (spsp_decode.hip).
    static const bool regions_on = getenv("SPSP_DEBUG_READ_BLOCK") == nullptr || getenv("SPSP_DEBUG_READ_BLOCK")[0] != '0';
    if (n >= 256 && regions_on) {
        if (ctx->h_read_regions.size() < workers) ctx->h_read_regions.resize(workers);
        std::vector<uint64_t> at(n, 0);                          // the payload's place in its thread's region
        auto range = [&](unsigned w) {
            spsp_ctx::ReadRegion& G = ctx->h_read_regions[w];
            size_t used = 0;
            auto room = [&](size_t more) -> bool {              // (grows by half: the places are offsets until the range is done)
                if (used + more + 64 <= G.cap) return true;
                size_t cap = std::max<size_t>(G.cap + G.cap / 2, used + more + 64);
                cap = (cap + 0xfffffu) & ~(size_t)0xfffffu;
                uint8_t* q = (uint8_t*)realloc(G.p, cap);
                if (!q) return false;
                G.p = q; G.cap = cap;
                return true;
            };
            struct Inflator { z_stream zs; bool live = false; ~Inflator() { if (live) inflateEnd(&zs); } };
            static thread_local Inflator I;
            std::vector<uint8_t> plain;
            const uint32_t i0 = (uint32_t)((uint64_t)n * w / workers), i1 = (uint32_t)((uint64_t)n * (w + 1) / workers);
            for (uint32_t i = i0; i < i1; ++i) {
                uint8_t* raw = nullptr; uint64_t raw_len = 0;
                rcs[i] = slurp(paths[i], &raw, &raw_len);
                if (rcs[i]) { errs[i] = spsp_last_error(); continue; }
                const bool gz = raw_len >= 18 && raw[0] == 0x1F && raw[1] == 0x8B;
                const bool zl = !gz && raw_len >= 2 && raw[0] == 0x78 && (raw[1] == 0x01 || raw[1] == 0x9C || raw[1] == 0xDA);
                bool placed = false;
                if (gz) {
                    // one member whose trailer tells the length (a forged one must not size a buffer: deflate never expands 1032-fold):
                    // inflated straight to its place
                    uint32_t isize; memcpy(&isize, raw + raw_len - 4, 4);
                    bool ok = (uint64_t)isize <= 1032ull * raw_len + 64 && raw_len < (1ull << 31) && room(isize);
                    if (ok) {
                        if (!I.live) { memset(&I.zs, 0, sizeof I.zs); ok = inflateInit2(&I.zs, 15 + 16) == Z_OK; I.live = ok; }
                        else ok = inflateReset2(&I.zs, 15 + 16) == Z_OK;
                    }
                    if (ok) {
                        uint8_t spill[8];
                        I.zs.next_in = raw; I.zs.avail_in = (uInt)raw_len;
                        I.zs.next_out = isize ? G.p + used : spill; I.zs.avail_out = isize;
                        int ret = inflate(&I.zs, Z_FINISH);
                        if (ret == Z_BUF_ERROR && I.zs.avail_out == 0) {   // the output is full: the trailer is still to be read
                            I.zs.next_out = spill; I.zs.avail_out = 0;
                            ret = inflate(&I.zs, Z_FINISH);
                        }
                        if (ret == Z_STREAM_END && I.zs.avail_in == 0 && I.zs.total_out == isize) { at[i] = used; lens[i] = isize; placed = true; }
                    }
                }
                if (!placed) {
                    // several members, a trailer that does not tell the truth, a zlib wrapper, a damaged file (the general reader and
                    // its error text), or plain text: appended all the same
                    const uint8_t* src = raw; uint64_t len = raw_len;
                    if (gz || zl) {
                        rcs[i] = inflate_all(raw, raw_len, plain);
                        if (rcs[i]) { errs[i] = spsp_last_error(); free(raw); continue; }
                        src = plain.data(); len = plain.size();
                    }
                    if (!room((size_t)len)) { set_error("out of host memory"); rcs[i] = SPSP_ERR_NOMEM; errs[i] = spsp_last_error(); free(raw); continue; }
                    if (len) memcpy(G.p + used, src, (size_t)len);
                    at[i] = used; lens[i] = len;
                }
                free(raw);
                used = (size_t)((used + lens[i] + 15) & ~(uint64_t)15);
            }
            for (uint32_t i = i0; i < i1; ++i) if (!rcs[i]) { datas[i] = G.p + at[i]; own[i] = 0; }
        };
        std::vector<std::thread> pool;
        for (unsigned w = 1; w < workers; ++w) pool.emplace_back(range, w);
        range(0);
        for (auto& th : pool) th.join();
    } else {
        on_threads([&](uint32_t i) {
            rcs[i] = spsp_read_file_host(paths[i], &datas[i], &lens[i]);
            if (rcs[i]) errs[i] = spsp_last_error();
        });
    }
    int rc = SPSP_OK;
    static const bool load_times = getenv("SPSP_DEBUG_DECODE_TIMES") != nullptr;
    if (load_times) fprintf(stderr, "[load] read + gunzip of %u files on %u threads %.4f s\n", n, workers, now_s() - t0);
    for (uint32_t i = 0; i < n && !rc; ++i)
        if (rcs[i]) { set_error("%s", errs[i].c_str()); rc = rcs[i]; }
    // k and m of the first header (every sketch is checked against them by the decoder)
    uint32_t k0 = 0, m0 = 0;
    if (!rc && n) {
        const uint8_t* nl = (const uint8_t*)memchr(datas[0], '\n', lens[0]);
        long skm = 0, mm = 0;
        if (nl) { char* e = nullptr; const std::string h((const char*)datas[0], nl - datas[0]); skm = strtol(h.c_str(), &e, 10); mm = strtol(e, &e, 10); }
        if (!nl || skm <= 0 || skm > 126 || mm <= 0 || mm > 15 || (skm + mm) / 2 > 63 || (skm + mm) / 2 < mm) { set_error("bad sketch header in '%s'", paths[0]); rc = SPSP_ERR_FORMAT; }
        else { m0 = (uint32_t)mm; k0 = (uint32_t)((skm + mm) / 2); }
    }
    L->k = k0; L->m = m0;
    // the merge's shared first-read buffer, in file order (see spsp_sketch_chain_host): phantom keys of empty sketches
    L->extra_has.assign(n, 0); L->extra_mn.assign(n, 0);
    if (!rc && n) {
        char buffer[16];
        memset(buffer, 'A', sizeof buffer);
        for (uint32_t i = 0; i < n && !rc; ++i) {
            int has = 0; uint32_t mn = 0; uint64_t lo = 0, hi = 0;
            rc = spsp_sketch_chain_host(datas[i], lens[i], k0, m0, buffer, &has, &mn, &lo, &hi);
            if (!rc && has) { L->extra_has[i] = 1; L->extra_mn[i] = mn; }
        }
    }
    if (load_times) fprintf(stderr, "[load] ... with the first-read chain %.4f s\n", now_s() - t0);
    // a common sampling rate: the headers' rates (read here, where the payloads lie anyway), as the thresholds they stand for
    L->rate_asked = rate != SPSP_RATE_AS_IS;
    if (!rc && n && L->rate_asked) {
        if (k0 == m0) { set_error("a common sampling rate cannot be applied to k == m sketches (k = m = %u)", k0); rc = SPSP_ERR_ARG; }
        std::vector<uint64_t> thr(n, 0);
        std::vector<double> rates(n, 0);
        double last_rate = 0; uint64_t last_thr = 0; bool have_last = false;
        for (uint32_t i = 0; i < n && !rc; ++i) {
            uint32_t ki = 0, mi = 0; uint64_t cnt = 0;
            rc = sketch_header_fields(datas[i], lens[i], &ki, &mi, &cnt, &rates[i], nullptr);
            if (rc) { const std::string why = spsp_last_error(); set_error("'%s': %s", paths[i], why.c_str()); break; }
            if (ki != k0 || mi != m0) { set_error("'%s' was made with k=%u m=%u, the first sketch with k=%u m=%u", paths[i], ki, mi, k0, m0); rc = SPSP_ERR_FORMAT; break; }
            if (!have_last || rates[i] != last_rate) { last_rate = rates[i]; last_thr = spsp_threshold_host(k0, m0, rates[i]); have_last = true; }   // (powl once per run of equal rates)
            thr[i] = last_thr;
        }
        if (!rc) {
            if (rate == SPSP_RATE_COARSEST) {
                uint32_t at = 0;
                for (uint32_t i = 1; i < n; ++i) if (thr[i] < thr[at]) at = i;
                L->ds_threshold = thr[at]; L->ds_rate = rates[at];
            } else { L->ds_threshold = spsp_threshold_host(k0, m0, rate); L->ds_rate = rate; }
            for (uint32_t i = 0; i < n && !rc; ++i) {
                if (thr[i] < L->ds_threshold) { set_error("cannot upsample: '%s' was sketched at rate %g, coarser than the common rate %g", paths[i], rates[i], L->ds_rate); rc = SPSP_ERR_ARG; }
                else if (thr[i] > L->ds_threshold) ++L->ds_brought;
            }
            L->ds_on = !rc && L->ds_brought > 0;                   // (every sketch already there: no pass)
        }
    }
    return rc;
}

double files_loaded(spsp_ctx* ctx, const LoadedSketches& L, uint32_t n, int chatter) {
    if (chatter && n) { printf("kmers evaluated are of length: %u minimizer size is %u\n", L.k, L.m); fflush(stdout); }   // :56
    const double t = now_s();
    ctx->stages.load_s += t - L.t0;
    return t;
}

int write_csv_gz(spsp_ctx* ctx, char* text, uint64_t len, const char* out_prefix, const char* suffix, double t_csv) {
    const double t = now_s();
    ctx->stages.csv_s += t - t_csv;
    const int rc = spsp_write_gz_host((std::string(out_prefix) + suffix).c_str(), (const uint8_t*)text, len, 1);   // level 1: Comparator.cpp:363,413
    ctx->stages.csv_gzip_s += now_s() - t;
    free(text);
    return rc;
}

void say_common_rate(const LoadedSketches& L, uint32_t n) {
    if (n && L.rate_asked) { printf("Sketches compared at sampling rate %g: %u of %u brought down to it\n", L.ds_rate, L.ds_brought, n); fflush(stdout); }
}

int write_key_sketches(uint32_t k, uint32_t m, double rate, const HostKeys& keys, const uint64_t* off, uint32_t n_out,
                       const std::function<std::string(uint32_t)>& name_of, const char* list_path) {
    std::string list;
    for (uint32_t i = 0; i < n_out; ++i) {
        const std::string path = name_of(i);
        list += path + "\n";
        uint8_t* payload = nullptr; uint64_t len = 0;
        const uint64_t a = off[i], c = off[i + 1] - off[i];
        int rc = spsp_sketch_from_keys_host(k, m, rate, keys.mn.data() + a, keys.lo.data() + a, k > 32 ? keys.hi.data() + a : nullptr, c, &payload, &len);
        if (rc) return rc;
        rc = spsp_write_gz_host(path.c_str(), payload, len, 9);
        free(payload);
        if (rc) return rc;
    }
    if (!list_path) return SPSP_OK;
    FILE* f = fopen(list_path, "wb");
    if (!f || fwrite(list.data(), 1, list.size(), f) != list.size() || fclose(f) != 0) { set_error("cannot write '%s'", list_path); return SPSP_ERR_IO; }
    return SPSP_OK;
}

// the threshold rule's arguments as a classification and a taxonomy call take them (what: the pass's name in the texts)
static int threshold_check(const char* what, uint32_t min_keys, uint32_t num, uint32_t den) {
    if (min_keys == 0) { set_error("%s: min_keys is 1 at the least", what); return SPSP_ERR_ARG; }
    if (den == 0 || num > den || den > kCfMaxDen) { set_error("%s threshold %u / %u: needs 0 <= num <= den, 1 <= den <= %u", what, num, den, kCfMaxDen); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

// spsp_classify.hip: what a classification call and the file driver refuse before anything else
int classify_check_args(uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den) {
    if (top == 0 || top > kCfMaxTop) { set_error("classification lists 1 .. %u matches per record (top = %u)", kCfMaxTop, top); return SPSP_ERR_ARG; }
    return threshold_check("classification", min_keys, num, den);
}

// spsp_taxonomy.hip: likewise
int taxonomy_check_args(uint32_t min_keys, uint32_t num, uint32_t den) { return threshold_check("taxonomy", min_keys, num, den); }

// What the record file drivers need no device for (spsp_classify.hip; DESIGN "What the record file drivers share")
void record_names_host(const uint8_t* text, uint64_t n, bool fastq, std::vector<std::string>* names) {
    uint64_t end = n;
    while (end && (text[end - 1] == '\n' || text[end - 1] == '\r')) --end;   // (FASTQ: the content without its trailing blank lines)
    uint64_t line = 0;
    for (uint64_t pos = 0; pos < (fastq ? end : n); ++line) {
        uint64_t stop = pos;
        while (stop < n && text[stop] != '\n') ++stop;
        const bool header = fastq ? line % 4 == 0 : text[pos] == '>';
        if (header) {
            uint64_t a = pos < stop ? pos + 1 : pos, z = a;   // (behind the '>' or '@')
            while (z < stop && text[z] != ' ' && text[z] != '\t' && text[z] != '\r') ++z;
            names->emplace_back((const char*)text + a, (size_t)(z - a));
        }
        pos = stop + 1;
    }
}

std::vector<uint32_t> records_batch_bounds(uint32_t n_rec) {
    std::vector<uint32_t> bounds;
    for (uint64_t r = 0; r < n_rec; r += 65535u) bounds.push_back((uint32_t)r);
    bounds.push_back(n_rec);
    return bounds;
}

int write_bytes(const char* path, const uint8_t* data, uint64_t len, int gz) {
    if (gz) return spsp_write_gz_host(path, data, len, 1);
    FILE* f = fopen(path, "wb");
    const bool wrote = f && fwrite(data, 1, (size_t)len, f) == len;
    if ((f && fclose(f) != 0) || !wrote) { set_error("cannot write '%s'", path); return SPSP_ERR_IO; }
    return SPSP_OK;
}

int record_files_check_args(const RecordFront& front, const RecordsAsk& ask) {
    const int tax = front.taxonomy ? 1 : 0;
    if (!front.ctx || !front.index_paths || !ask.records_paths || !ask.records_paths[0] || !ask.out_prefix || (tax && !front.lineages_path) ||
        (front.paired && !ask.mates_path) || (ask.mode == kRmWindows && !ask.what)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (front.n_ref == 0 || front.n_ref > 65535) { set_error("a classification index takes 1 .. 65535 references (n = %u)", front.n_ref); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = tax ? taxonomy_check_args(front.min_keys, front.num, front.den) : classify_check_args(front.top, front.min_keys, front.num, front.den))) return rc;
    // (the word, before any file is read; a taxonomy's extract word names its node once the tree is)
    if (ask.mode == kRmExtract && (rc = spsp_extract_word_check_host(ask.what, tax, tax ? 0xffffffffu : front.n_ref))) return rc;
    if (ask.mode == kRmSplit && (rc = spsp_split_word_check_host(ask.what, tax))) return rc;
    if (ask.mode == kRmWindows && (rc = spsp_windows_word_check_host(ask.what, tax))) return rc;
    if (ask.mode == kRmWindows && (ask.window == 0 || ask.window > kWnMaxWidth)) {   // (against k: once the sketches' headers are read, behind the ingest)
        set_error("windows: the width must be k .. %llu (width = %llu)", (unsigned long long)kWnMaxWidth, (unsigned long long)ask.window);
        return SPSP_ERR_ARG;
    }
    if (ask.mode != kRmWindows && (ask.smooth || ask.segments_what)) { set_error("segments: smoothing and the segments' text belong to a windowed run"); return SPSP_ERR_ARG; }
    if (ask.smooth > 0x7fffffffu) { set_error("segments: the smoothing must be 0 .. 2147483647 (q = %u)", ask.smooth); return SPSP_ERR_ARG; }
    // (the selection's word likewise; <b> of a taxonomy against the nodes once the tree is read, in the pass's prelude)
    if (ask.segments_what && (rc = segments_ask_check(ask, tax, tax ? 0u : front.n_ref + 1))) return rc;
    return SPSP_OK;
}

int segments_ask_check(const RecordsAsk& ask, int taxonomy, uint32_t n_bins) {
    if (!ask.segments_what) return SPSP_OK;
    if (strchr(ask.segments_what, ':')) { set_error("segments: '%s' is no word (all, called, none, call=<b>, not=<b>, major, minor)", ask.segments_what); return SPSP_ERR_ARG; }
    if (ask.segments_min >> 63) { set_error("segments: the least length must be below 2^63"); return SPSP_ERR_ARG; }
    return spsp_segments_word_check_host(ask.segments_what, taxonomy, n_bins);
}

int give_rows_all(const RowsGift* gifts, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!gifts[i].out) continue;
        void* p = malloc(gifts[i].bytes ? gifts[i].bytes : 1);
        if (!p) {
            for (size_t j = 0; j < n; ++j) if (gifts[j].out) { if (j < i) free(*gifts[j].out); *gifts[j].out = nullptr; }
            set_error("out of host memory");
            return SPSP_ERR_NOMEM;
        }
        if (gifts[i].bytes) memcpy(p, gifts[i].rows, gifts[i].bytes);
        *gifts[i].out = p;
    }
    return SPSP_OK;
}
}  // namespace spsp

namespace {
int clamp_chatter(int chatter) { return chatter < 0 ? 0 : (chatter > 2 ? 2 : chatter); }

// a CSV writer's text as the caller's to spsp_free
int text_out(const std::string& out, char** text, uint64_t* len) {
    char* buf = (char*)malloc(out.size() ? out.size() : 1);
    if (!buf) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    memcpy(buf, out.data(), out.size());
    *text = buf; *len = out.size();
    return SPSP_OK;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ the linkage tree's helpers
namespace {
inline uint64_t tree_under(int metric, const uint64_t* card, uint32_t a, uint32_t b, uint64_t x) {
    return metric == SPSP_CLUSTER_JACCARD ? card[a] + card[b] - x : std::min(card[a], card[b]);
}
int tree_check_metric(int metric) {
    if (metric == SPSP_CLUSTER_JACCARD || metric == SPSP_CLUSTER_CONTAINMENT) return SPSP_OK;
    set_error("tree metric %d: 0 (Jaccard) or 1 (containment)", metric);
    return SPSP_ERR_ARG;
}
int tree_check_rows(const spsp_tree_row* rows, uint64_t n_rows, uint32_t n) {
    if (n_rows >= n) { set_error("%llu tree rows over %u sketches: a forest has n - 1 at the most", (unsigned long long)n_rows, n); return SPSP_ERR_ARG; }
    for (uint64_t r = 0; r < n_rows; ++r)
        if (rows[r].a >= rows[r].b || rows[r].b >= n) { set_error("tree row %llu does not name two sketches a < b < n", (unsigned long long)r); return SPSP_ERR_ARG; }
    return SPSP_OK;
}
// union-find over the sketches on the host: the root of a set is its first-listed member
struct TreeSets {
    std::vector<uint32_t> up;
    explicit TreeSets(uint32_t n) : up(n) { for (uint32_t i = 0; i < n; ++i) up[i] = i; }
    uint32_t find(uint32_t x) {
        uint32_t r = x;
        while (up[r] != r) r = up[r];
        while (up[x] != r) { const uint32_t next = up[x]; up[x] = r; x = next; }
        return r;
    }
    uint32_t unite(uint32_t a, uint32_t b) { if (a > b) std::swap(a, b); up[b] = a; return a; }   // of two roots -> the new root
};
void newick_leaf(std::string& out, const char* name) {
    out += '\'';
    for (const char* c = name; *c; ++c) { if (*c == '\'') out += '\''; out += *c; }
    out += '\'';
}
}  // namespace

// the forest's cell words in any order -> the rows in the rule's order (the better fraction first by 128-bit cross products, then
// the smaller (i, j)), each with the size of the cluster its merge makes
int spsp::tree_rows_host(const uint64_t* forest, uint64_t n_forest, const uint64_t* card, uint32_t n, int metric, spsp_tree_row* rows) {
    struct Edge { uint64_t word, u; };
    std::vector<Edge> edges(n_forest);
    for (uint64_t e = 0; e < n_forest; ++e) {
        const uint64_t c = forest[e];
        const uint32_t a = (uint32_t)(c >> 48), b = (uint32_t)(c >> 32) & 0xffffu;
        if (a >= b || b >= n) { set_error("forest edge %llu does not name two sketches a < b < n", (unsigned long long)e); return SPSP_ERR_ARG; }
        edges[e] = Edge{c, tree_under(metric, card, a, b, c & 0xffffffffull)};
    }
    std::sort(edges.begin(), edges.end(), [](const Edge& p, const Edge& q) {
        const u128 l = (u128)(p.word & 0xffffffffull) * q.u, r = (u128)(q.word & 0xffffffffull) * p.u;
        return l != r ? l > r : (p.word >> 32) < (q.word >> 32);
    });
    TreeSets sets(n);
    std::vector<uint32_t> size(n, 1);
    for (uint64_t e = 0; e < n_forest; ++e) {
        const uint64_t c = edges[e].word;
        const uint32_t a = (uint32_t)(c >> 48), b = (uint32_t)(c >> 32) & 0xffffu, ra = sets.find(a), rb = sets.find(b);
        if (ra == rb) { set_error("forest edge (%u, %u) closes a cycle", a, b); return SPSP_ERR_ARG; }
        const uint32_t total = size[ra] + size[rb];
        size[sets.unite(ra, rb)] = total;
        rows[e].a = a; rows[e].b = b; rows[e].size = total; rows[e].reserved = 0; rows[e].shared = c & 0xffffffffull;
    }
    return SPSP_OK;
}

extern "C" {

// chatter: 0 = silent; 1 = the stdout lines of the reference's all-versus-all run (Comparator.cpp:56,69,364,414,
// 503,509); 2 = those of its query run (:56,69,364,414)
// more / n_more: all contexts of a multi-device call (more[0] == ctx): the comparison is then split by key over them
// rate: as load_sketch_files takes it
static int compare_files_impl(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision,
                              double min_threshold, const char* out_prefix, int chatter, double rate, spsp_ctx* const* more = nullptr, uint32_t n_more = 0) {
    if (!ctx || !paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    spsp::LoadedSketches L;
    int rc = spsp::load_sketch_files(ctx, paths, n, rate, &L);
    if (rc) { ctx->stages.compare_s += now_s() - L.t0; return rc; }
    double t0 = spsp::files_loaded(ctx, L, n, chatter), t1;
    // the pair matrix: zero pages from calloc (400 MB at 10^4 sketches: touched only where a row is written or read)
    struct Matrix { uint32_t* p = nullptr; ~Matrix() { free(p); } uint32_t* data() { return p; }
                    int zero(size_t cells) { free(p); p = (uint32_t*)calloc(cells ? cells : 1, 4); return p ? SPSP_OK : SPSP_ERR_NOMEM; } } inter;
    bool mirrored = false;                                    // both triangles filled
    std::vector<uint64_t> cells;                              // ... or no matrix at all: a large comparison comes back as its non-zero cells
    const bool as_cells = n >= 1024 && n <= 65535;            // (the printers then work from the cells: no n x n matrix on the host)
    std::vector<uint64_t> card(n, 0);
    uint32_t kk = 0, mm2 = 0;
    if (!as_cells && (rc = inter.zero((size_t)n * n))) set_error("out of host memory");
    else if (n_more > 1) rc = spsp::compare_payloads_multi(more, n_more, L.data.data(), L.len.data(), n, L.extra_has.data(), L.extra_mn.data(), n_query, L.threshold(),
                                                           &kk, &mm2, inter.data(), card.data(), &mirrored, as_cells ? &cells : nullptr);
    else rc = spsp::compare_payloads_impl(ctx, L.data.data(), L.len.data(), n, L.extra_has.data(), L.extra_mn.data(), n_query, L.threshold(), &kk, &mm2,
                                          inter.data(), card.data(), &mirrored, as_cells ? &cells : nullptr);
    L.release();
    t1 = now_s(); ctx->stages.compare_s += t1 - t0;
    if (rc) return rc;
    if (chatter) {
        printf("Comparisons done\n");                                                         // :69
        if (chatter == 1) std::cout << "Comparisons lasted " << (t1 - L.t0) << " sec" << std::endl;   // :503 (cout's default float format)
        fflush(stdout);
    }
    const double t_middle = t1;
    for (int jac = 0; jac < 2 && !rc; ++jac) {
        char* text = nullptr; uint64_t len = 0;
        t0 = now_s();
        if (chatter) { printf(jac ? "Jackard index dump\n" : "Containement index dump \n"); fflush(stdout); }   // :364, :414
        const char* suffix = jac ? "_jaccard.csv.gz" : "_containment.csv.gz";
        if (as_cells) {
            // rows formatted from the cells and deflated block by block on the workers, level 1 (Comparator.cpp:363,413)
            double tt[2] = {0, 0};
            rc = csv_cells_impl(jac, paths, n, n_query, cells, card.data(), precision, min_threshold, nullptr, nullptr, (std::string(out_prefix) + suffix).c_str(), 1, tt);
            ctx->stages.csv_s += tt[0]; ctx->stages.csv_gzip_s += tt[1];
            continue;
        }
        rc = csv_impl(jac, paths, n, n_query, inter.data(), card.data(), precision, min_threshold, &text, &len, mirrored);
        if (rc) { ctx->stages.csv_s += now_s() - t0; break; }
        rc = spsp::write_csv_gz(ctx, text, len, out_prefix, suffix, t0);
    }
    if (!rc && chatter == 1) std::cout << "Jaccard output lasted " << (now_s() - t_middle) << " sec" << std::endl;   // :509
    if (!rc && chatter) spsp::say_common_rate(L, n);
    return rc;
}

int spsp_gather_csv_host(const spsp_gather_row* rows, uint64_t n_rows, const char* const* names, uint32_t n, uint32_t n_query,
                         const uint64_t* card, int precision, char** text, uint64_t* len) {
    if (!text || !len || (n_rows && (!rows || !names || !card))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::string out = "query,rank,match,intersect,unique,f_unique_query,f_match,remaining\n";
    char num[64];
    for (uint64_t i = 0; i < n_rows; ++i) {
        const spsp_gather_row& r = rows[i];
        if (r.query >= n_query || r.match < n_query || r.match >= n) { set_error("gather row %llu names a sketch outside the lists", (unsigned long long)i); return SPSP_ERR_ARG; }
        out += names[r.query]; out += ',';
        out += std::to_string(r.rank); out += ',';
        out += names[r.match]; out += ',';
        out += std::to_string(r.intersect); out += ',';
        out += std::to_string(r.unique); out += ',';
        out.append(num, format_g(num, sizeof num, precision, (double)r.unique / (double)card[r.query])); out += ',';
        out.append(num, format_g(num, sizeof num, precision, (double)r.intersect / (double)card[r.match])); out += ',';
        out += std::to_string(r.remaining); out += '\n';
    }
    return text_out(out, text, len);
}

int spsp_cluster_csv_host(const spsp_cluster_row* rows, const char* const* names, uint32_t n, const uint64_t* card, int metric, int precision,
                          char** text, uint64_t* len) {
    if (!text || !len || (n && (!rows || !names || !card))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (metric != SPSP_CLUSTER_JACCARD && metric != SPSP_CLUSTER_CONTAINMENT) { set_error("cluster metric %d: 0 (Jaccard) or 1 (containment)", metric); return SPSP_ERR_ARG; }
    std::string out = "sketch,cluster,representative,size,keys,shared,score\n";
    char num[64];
    for (uint32_t i = 0; i < n; ++i) {
        const spsp_cluster_row& r = rows[i];
        if (r.representative >= n || rows[r.representative].cluster != r.cluster) {
            set_error("cluster row %u names a representative outside %s", i, r.representative >= n ? "the list" : "its own cluster");
            return SPSP_ERR_ARG;
        }
        const uint64_t ci = card[i], cr = card[r.representative];
        double score = 1.0;                                    // (printed only: the integer test has decided)
        if (r.representative != i) {
            const double under = metric == SPSP_CLUSTER_JACCARD ? (double)(ci + cr - r.shared) : (double)std::min(ci, cr);
            score = r.shared ? (double)r.shared / under : 0.0;
        }
        out += names[i]; out += ',';
        out += std::to_string(r.cluster); out += ',';
        out += names[r.representative]; out += ',';
        out += std::to_string(r.size); out += ',';
        out += std::to_string(ci); out += ',';
        out += std::to_string(r.shared); out += ',';
        out.append(num, format_g(num, sizeof num, precision, score)); out += '\n';
    }
    return text_out(out, text, len);
}

int spsp_neighbours_csv_host(const spsp_neighbour_row* rows, uint64_t n_rows, const uint32_t* passing, const char* const* names, uint32_t n,
                             uint32_t n_query, const uint64_t* card, int metric, int precision, char** text, uint64_t* len) {
    if (!text || !len || (n_rows && (!rows || !names || !card))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (metric != SPSP_NEIGHBOUR_JACCARD && metric != SPSP_NEIGHBOUR_CONTAINMENT && metric != SPSP_NEIGHBOUR_CONTAINED) {
        set_error("neighbour metric %d: 0 (Jaccard), 1 (the larger containment) or 2 (the row's containment in the partner)", metric);
        return SPSP_ERR_ARG;
    }
    std::string out = "sketch,rank,neighbour,shared,keys,neighbour_keys,score,passing\n";
    char num[64];
    const bool all = n_query == n;
    for (uint64_t i = 0; i < n_rows; ++i) {
        const spsp_neighbour_row& r = rows[i];
        if (r.sketch >= n_query || r.sketch >= n || r.neighbour >= n || (!all && r.neighbour < n_query) || r.neighbour == r.sketch) {
            set_error("neighbour row %llu names a sketch outside the lists (or a query, or the sketch itself, as the neighbour)", (unsigned long long)i);
            return SPSP_ERR_ARG;
        }
        const uint64_t cr = card[r.sketch], cp = card[r.neighbour];
        const uint64_t under = metric == SPSP_NEIGHBOUR_JACCARD ? cr + cp - r.shared : metric == SPSP_NEIGHBOUR_CONTAINMENT ? std::min(cr, cp) : cr;
        out += names[r.sketch]; out += ',';
        out += std::to_string(r.rank); out += ',';
        out += names[r.neighbour]; out += ',';
        out += std::to_string(r.shared); out += ',';
        out += std::to_string(cr); out += ',';
        out += std::to_string(cp); out += ',';
        out.append(num, format_g(num, sizeof num, precision, (double)r.shared / (double)under)); out += ',';   // (printed only: the integer order has decided)
        out += std::to_string(passing ? passing[r.sketch] : 0u); out += '\n';
    }
    return text_out(out, text, len);
}

int spsp_prevalence_csv_host(const spsp_prevalence_row* rows, uint32_t n_rows, const char* const* names, const uint64_t* card, int precision,
                             char** text, uint64_t* len) {
    if (!text || !len || (n_rows && (!rows || !names || !card))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::string out = "sketch,keys,core,shell,unique,absent,f_core,mean_holders\n";
    char num[64];
    for (uint32_t i = 0; i < n_rows; ++i) {
        const spsp_prevalence_row& r = rows[i];
        const uint64_t keys = card[i];
        if (r.core + r.shell + r.unique + r.absent != keys) { set_error("prevalence row %u: its classes do not add up to the sketch's %llu keys", i, (unsigned long long)keys); return SPSP_ERR_ARG; }
        out += names[i]; out += ',';
        out += std::to_string(keys); out += ',';
        out += std::to_string(r.core); out += ',';
        out += std::to_string(r.shell); out += ',';
        out += std::to_string(r.unique); out += ',';
        out += std::to_string(r.absent); out += ',';
        out.append(num, format_g(num, sizeof num, precision, keys ? (double)r.core / (double)keys : 0.0)); out += ',';
        out.append(num, format_g(num, sizeof num, precision, keys ? (double)r.holders / (double)keys : 0.0)); out += '\n';
    }
    return text_out(out, text, len);
}

int spsp_spectrum_csv_host(const uint64_t* spectrum, uint32_t n_ref, char** text, uint64_t* len) {
    if (!text || !len || !spectrum) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    uint64_t cumulative = 0;
    for (uint32_t t = 1; t <= n_ref; ++t) cumulative += spectrum[t];
    std::string out = "holders,keys,cumulative\n";
    for (uint32_t t = 1; t <= n_ref; ++t) {
        if (spectrum[t]) { out += std::to_string(t); out += ','; out += std::to_string(spectrum[t]); out += ','; out += std::to_string(cumulative); out += '\n'; }
        cumulative -= spectrum[t];
    }
    return text_out(out, text, len);
}

// ------------------------------------------------------------------------------------------------ accumulation
// what the pass kernel of spsp_accumulation.hip is launched with for n sketches.  LDS of a workgroup: kAcLdsBytes less a bitmap of
// kAcBitmapBits per wave; an order costs its rank table (2 bytes per sketch, n rounded up to even) and 4 bytes per rank of the
// window.  While whole orders fit with a window of all n ranks: as many as fit, rounded down to a power of two, kAcMaxGroup at the
// most, ONE window.  Beyond that (n > 25 941): one order, and the window is what the rank table leaves
int spsp_accumulation_plan_host(uint32_t n, uint32_t* group, uint32_t* window, uint32_t* bitmap_bits, uint32_t* cut) {
    if (n == 0 || n > 65535) { set_error("accumulation takes 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    using namespace spsp;
    const uint32_t budget = kAcLdsBytes - (kAcPassThreads / 64) * (kAcBitmapBits / 8), rank_bytes = 2u * ((n + 1u) & ~1u);
    const uint32_t fit = budget / (rank_bytes + 4u * n);
    uint32_t g = 1, w = n;
    if (fit >= 1) { while (g * 2 <= fit && g * 2 <= kAcMaxGroup) g *= 2; }
    else w = (budget - rank_bytes) / 4u;
    if (group) *group = g;
    if (window) *window = w;
    if (bitmap_bits) *bitmap_bits = kAcBitmapBits;
    if (cut) *cut = kAcCut;
    return SPSP_OK;
}

int spsp_accumulation_orders_host(uint32_t n, uint32_t n_orders, uint64_t seed, uint32_t* orders) {
    if (!orders) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n == 0 || n > 65535) { set_error("accumulation takes 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (n_orders == 0 || n_orders > 1024) { set_error("accumulation takes 1 .. 1024 orders (%u)", n_orders); return SPSP_ERR_ARG; }
    uint64_t s = seed;
    const auto draw = [&s]() {                             // splitmix64
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    for (uint32_t p = 0; p < n_orders; ++p) {
        uint32_t* a = orders + (size_t)p * n;
        for (uint32_t i = 0; i < n; ++i) a[i] = i;
        if (p == 0) continue;                              // order 0: the list order
        for (uint32_t i = n - 1; i >= 1; --i) {
            const uint64_t b = (uint64_t)i + 1, rem = (0ull - b) % b;   // rem = 2^64 mod b: draws from 2^64 - rem on are drawn again
            uint64_t z = draw();
            while (rem && z >= 0ull - rem) z = draw();
            std::swap(a[i], a[z % b]);
        }
    }
    return SPSP_OK;
}

int spsp_accumulation_csv_host(const spsp_accumulation_row* rows, uint32_t n, uint32_t n_orders, int precision, char** text, size_t* len) {
    if (!text || !len || !rows) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n == 0 || n > 65535) { set_error("accumulation takes 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (n_orders == 0 || n_orders > 1024) { set_error("accumulation takes 1 .. 1024 orders (%u)", n_orders); return SPSP_ERR_ARG; }
    typedef unsigned __int128 u128;
    const double P = (double)n_orders;
    std::string out = "genomes,pan_min,pan_mean,pan_max,core_min,core_mean,core_max,new_mean,pan_listed,core_listed\n";
    char num[64];
    uint64_t before = 0;                                   // pan_sum(j - 1)
    for (uint32_t j = 0; j < n; ++j) {
        const spsp_accumulation_row& r = rows[j];
        const char* why = nullptr;
        if (r.pan_min > r.pan_max || r.core_min > r.core_max) why = "a minimum above its maximum";
        else if ((u128)r.pan_sum < (u128)n_orders * r.pan_min || (u128)r.pan_sum > (u128)n_orders * r.pan_max ||
                 (u128)r.core_sum < (u128)n_orders * r.core_min || (u128)r.core_sum > (u128)n_orders * r.core_max) why = "a sum that its orders' minimum and maximum do not allow";
        else if (j && r.pan_min < rows[j - 1].pan_min) why = "pan_min falls";
        else if (j && r.core_max > rows[j - 1].core_max) why = "core_max rises";
        else if (r.pan_first < r.pan_min || r.pan_first > r.pan_max || r.core_first < r.core_min || r.core_first > r.core_max) why = "the listed order's value outside [min, max]";
        if (why) { set_error("accumulation row %u (%u genomes) is not a step of a curve: %s", j, j + 1, why); return SPSP_ERR_ARG; }
        const double grown = r.pan_sum >= before ? (double)(r.pan_sum - before) : -(double)(before - r.pan_sum);
        before = r.pan_sum;
        out += std::to_string(j + 1); out += ',';
        out += std::to_string(r.pan_min); out += ',';
        out.append(num, format_g(num, sizeof num, precision, (double)r.pan_sum / P)); out += ',';
        out += std::to_string(r.pan_max); out += ',';
        out += std::to_string(r.core_min); out += ',';
        out.append(num, format_g(num, sizeof num, precision, (double)r.core_sum / P)); out += ',';
        out += std::to_string(r.core_max); out += ',';
        out.append(num, format_g(num, sizeof num, precision, grown / P)); out += ',';
        out += std::to_string(r.pan_first); out += ',';
        out += std::to_string(r.core_first); out += '\n';
    }
    uint64_t l = 0;
    const int rc = text_out(out, text, &l);
    *len = (size_t)l;
    return rc;
}

// ------------------------------------------------------------------------------------------------ groups
// a labels file: one label per line in list order, groups numbered by first appearance
int spsp_groups_labels_host(const char* text, uint64_t len, uint32_t n, uint32_t* group, uint32_t* n_groups, char** names, uint64_t* names_len) {
    if (names) *names = nullptr;
    if (names_len) *names_len = 0;
    if (n_groups) *n_groups = 0;
    if ((!text && len) || !group || !n_groups) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n == 0 || n > 65535) { set_error("groups take 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    std::unordered_map<std::string, uint32_t> seen;
    std::string blob;
    uint64_t line = 0, pos = 0;
    while (pos < len) {
        uint64_t end = pos;
        while (end < len && text[end] != '\n') ++end;
        uint64_t stop = end;
        if (stop > pos && text[stop - 1] == '\r') --stop;  // ("\r\n" is tolerated)
        ++line;
        if (line > n) { set_error("labels: line %llu: more labels than the %u sketches", (unsigned long long)line, n); return SPSP_ERR_ARG; }
        if (stop == pos) { set_error("labels: line %llu: an empty label", (unsigned long long)line); return SPSP_ERR_ARG; }
        for (uint64_t q = pos; q < stop; ++q) {
            const unsigned char c = (unsigned char)text[q];
            if (c == ',' || c == '"' || c < 0x20 || c == 0x7f) {
                set_error("labels: line %llu: a label holds ',', '\"' or a control character (byte 0x%02x)", (unsigned long long)line, (unsigned)c);
                return SPSP_ERR_ARG;
            }
        }
        const std::string label(text + pos, (size_t)(stop - pos));
        const auto it = seen.find(label);
        if (it != seen.end()) group[line - 1] = it->second;
        else {
            const uint32_t g = (uint32_t)seen.size();
            seen.emplace(label, g);
            group[line - 1] = g;
            blob.append(label); blob.push_back('\0');
        }
        pos = end + 1;                                     // (the final newline is optional: nothing behind it is no line)
    }
    if (line != n) { set_error("labels: line %llu: the file ends after %llu label(s), %u sketches are listed", (unsigned long long)(line + 1), (unsigned long long)line, n); return SPSP_ERR_ARG; }
    *n_groups = (uint32_t)seen.size();
    if (names) {
        uint64_t l = 0;
        const int rc = text_out(blob, names, &l);
        if (rc) return rc;
        if (names_len) *names_len = l;
    }
    return SPSP_OK;
}

int spsp_groups_bounds_host(const uint32_t* group, uint32_t n, uint32_t n_groups, uint32_t num, uint32_t den, uint32_t onum, uint32_t oden,
                            uint32_t* size, uint32_t* in_min, uint32_t* out_max) {
    if (n == 0 || n > 65535) { set_error("groups take 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (n_groups == 0 || n_groups > n) { set_error("groups: %u groups of %u sketches (1 .. n; every group has a member)", n_groups, n); return SPSP_ERR_ARG; }
    if (!group) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (num == 0 || num > den || den > 1000000) { set_error("groups: inside threshold %u / %u: needs 1 <= num <= den <= 1000000", num, den); return SPSP_ERR_ARG; }
    if (onum > oden || oden == 0 || oden > 1000000) { set_error("groups: outside tolerance %u / %u: needs 0 <= onum <= oden, 1 <= oden <= 1000000", onum, oden); return SPSP_ERR_ARG; }
    std::vector<uint32_t> members(n_groups, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (group[i] >= n_groups) { set_error("groups: sketch %u has label %u, there are %u groups", i, group[i], n_groups); return SPSP_ERR_ARG; }
        ++members[group[i]];
    }
    for (uint32_t c = 0; c < n_groups; ++c)
        if (members[c] == 0) { set_error("groups: group %u has no member", c); return SPSP_ERR_ARG; }
    for (uint32_t c = 0; c < n_groups; ++c) {
        if (size) size[c] = members[c];
        if (in_min) in_min[c] = (uint32_t)(((uint64_t)num * members[c] + den - 1) / den);     // h_c * den >= num * size_c
        if (out_max) out_max[c] = (uint32_t)((uint64_t)onum * (n - members[c]) / oden);       // (h - h_c) * oden <= onum * (n - size_c)
    }
    return SPSP_OK;
}

int spsp_groups_csv_host(const spsp_group_row* rows, uint32_t n_groups, const char* const* group_names, int precision, char** text, uint64_t* len) {
    if (!text || !len || !rows || !group_names) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_groups == 0 || n_groups > 65535) { set_error("groups: %u groups (1 .. 65535)", n_groups); return SPSP_ERR_ARG; }
    std::string out = "group,members,keys,present,core,exclusive,marker,f_core,f_marker\n";
    char num[64];
    for (uint32_t c = 0; c < n_groups; ++c) {
        const spsp_group_row& r = rows[c];
        const char* why = r.core > r.present ? "more core keys than present keys" : r.marker > r.core ? "more marker keys than core keys" :
                          r.exclusive > r.present ? "more exclusive keys than present keys" : nullptr;
        if (why) { set_error("group row %u cannot be a group's counts: %s", c, why); return SPSP_ERR_ARG; }
        out += group_names[c]; out += ',';
        out += std::to_string(r.members); out += ',';
        out += std::to_string(r.entries); out += ',';
        out += std::to_string(r.present); out += ',';
        out += std::to_string(r.core); out += ',';
        out += std::to_string(r.exclusive); out += ',';
        out += std::to_string(r.marker); out += ',';
        out.append(num, format_g(num, sizeof num, precision, r.present ? (double)r.core / (double)r.present : 0.0)); out += ',';
        out.append(num, format_g(num, sizeof num, precision, r.core ? (double)r.marker / (double)r.core : 0.0)); out += '\n';
    }
    return text_out(out, text, len);
}

int spsp_groups_members_csv_host(const spsp_group_member_row* members, uint32_t n, const char* const* sketch_names, const uint32_t* group,
                                 const uint64_t* card, const spsp_group_row* rows, uint32_t n_groups, const char* const* group_names, int precision,
                                 char** text, uint64_t* len) {
    if (!text || !len || !members || !sketch_names || !group || !card || !rows || !group_names) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n == 0 || n > 65535) { set_error("groups take 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (n_groups == 0 || n_groups > n) { set_error("groups: %u groups of %u sketches (1 .. n; every group has a member)", n_groups, n); return SPSP_ERR_ARG; }
    std::string out = "sketch,group,keys,core,exclusive,marker,f_core,f_marker\n";
    char num[64];
    for (uint32_t i = 0; i < n; ++i) {
        const spsp_group_member_row& r = members[i];
        if (group[i] >= n_groups) { set_error("member row %u has label %u, there are %u groups", i, group[i], n_groups); return SPSP_ERR_ARG; }
        const spsp_group_row& g = rows[group[i]];
        const uint64_t keys = card[i];
        const char* why = (r.core > keys || r.exclusive > keys || r.marker > keys) ? "more keys of a kind than the sketch holds" :
                          r.marker > r.core ? "more marker keys than core keys" :
                          (r.core > g.core || r.exclusive > g.exclusive || r.marker > g.marker) ? "more keys of a kind than its group has" : nullptr;
        if (why) { set_error("member row %u cannot be a sketch's counts: %s", i, why); return SPSP_ERR_ARG; }
        out += sketch_names[i]; out += ',';
        out += group_names[group[i]]; out += ',';
        out += std::to_string(keys); out += ',';
        out += std::to_string(r.core); out += ',';
        out += std::to_string(r.exclusive); out += ',';
        out += std::to_string(r.marker); out += ',';
        out.append(num, format_g(num, sizeof num, precision, keys ? (double)r.core / (double)keys : 0.0)); out += ',';
        out.append(num, format_g(num, sizeof num, precision, g.marker ? (double)r.marker / (double)g.marker : 0.0)); out += '\n';
    }
    return text_out(out, text, len);
}

// ------------------------------------------------------------------------------------------------ classification
// what routes a record of spsp_classify.hip from one form to the other: the constants of spsp_internal.h
int spsp_classify_plan_host(uint32_t n_ref, uint32_t top, uint32_t* small_work, uint32_t* lds_refs, uint32_t* counters_in_lds, uint32_t* list_cut) {
    using namespace spsp;
    if (n_ref == 0 || n_ref > 65535) { set_error("a classification index takes 1 .. 65535 references (n = %u)", n_ref); return SPSP_ERR_ARG; }
    if (top == 0 || top > kCfMaxTop) { set_error("classification lists 1 .. %u matches per record (top = %u)", kCfMaxTop, top); return SPSP_ERR_ARG; }
    if (small_work) *small_work = kCfSmallWork;
    if (lds_refs) *lds_refs = kCfLdsRefs;
    if (counters_in_lds) *counters_in_lds = n_ref <= kCfLdsRefs ? 1u : 0u;
    if (list_cut) *list_cut = kCfListCut;
    return SPSP_OK;
}

// a record's row and matches that cannot be a classification's: why, or null
static const char* classify_row_wrong(const spsp_classify_record& r, const spsp_classify_hit* h, uint32_t n_ref, uint32_t top) {
    if (r.listed > top || r.listed > r.passing) return "more matches listed than min(top, passing)";
    if (r.hit_keys > r.keys) return "more hit keys than keys";
    for (uint32_t i = 0; i < r.listed; ++i) {
        if (h[i].reference >= n_ref) return "a match names a reference outside the index";
        if (h[i].shared > r.hit_keys) return "a match shares more keys than the record has hit keys";
        if (h[i].shared == 0) return "a listed match shares no key";
        if (i && (h[i].shared > h[i - 1].shared || (h[i].shared == h[i - 1].shared && h[i].reference <= h[i - 1].reference))) return "matches out of order";
    }
    return nullptr;
}

static int classify_csv_args(const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records, const char* const* ref_names, uint32_t n_ref,
                             uint32_t top, char** text, uint64_t* len) {
    if (!text || !len || !ref_names || (n_records && (!records || !hits))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_ref == 0 || n_ref > 65535) { set_error("a classification index takes 1 .. 65535 references (n = %u)", n_ref); return SPSP_ERR_ARG; }
    if (top == 0 || top > spsp::kCfMaxTop) { set_error("classification lists 1 .. %u matches per record (top = %u)", spsp::kCfMaxTop, top); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

int spsp_classify_csv_host(const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records, const char* const* record_names,
                           const char* const* ref_names, uint32_t n_ref, uint32_t top, int precision, char** text, uint64_t* len) {
    if (const int rc = classify_csv_args(records, hits, n_records, ref_names, n_ref, top, text, len)) return rc;
    if (n_records && !record_names) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::string out = "record,name,length,keys,hit_keys,rank,match,shared,f_shared,passing\n";
    char num[64];
    for (uint64_t r = 0; r < n_records; ++r) {
        const spsp_classify_record& rec = records[r];
        const spsp_classify_hit* h = hits + r * top;
        if (const char* why = classify_row_wrong(rec, h, n_ref, top)) { set_error("classification record %llu contradicts itself: %s", (unsigned long long)r, why); return SPSP_ERR_ARG; }
        const std::string front = std::to_string(r) + ',' + record_names[r] + ',' + std::to_string(rec.length) + ',' + std::to_string(rec.keys) + ',' +
                                  std::to_string(rec.hit_keys) + ',';
        const std::string back = ',' + std::to_string(rec.passing) + '\n';
        if (rec.listed == 0) { out += front; out += "0,,0,0"; out += back; continue; }
        for (uint32_t i = 0; i < rec.listed; ++i) {
            out += front;
            out += std::to_string(i + 1); out += ',';
            out += ref_names[h[i].reference]; out += ',';
            out += std::to_string(h[i].shared); out += ',';
            out.append(num, format_g(num, sizeof num, precision, rec.keys ? (double)h[i].shared / (double)rec.keys : 0.0));
            out += back;
        }
    }
    return text_out(out, text, len);
}

int spsp_classify_summary_csv_host(const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records, const char* const* ref_names,
                                   uint32_t n_ref, uint32_t top, char** text, uint64_t* len) {
    if (const int rc = classify_csv_args(records, hits, n_records, ref_names, n_ref, top, text, len)) return rc;
    std::vector<uint64_t> best(n_ref, 0), bases(n_ref, 0), keys(n_ref, 0), listed(n_ref, 0);
    uint64_t none = 0, none_bases = 0;
    for (uint64_t r = 0; r < n_records; ++r) {
        const spsp_classify_record& rec = records[r];
        const spsp_classify_hit* h = hits + r * top;
        if (const char* why = classify_row_wrong(rec, h, n_ref, top)) { set_error("classification record %llu contradicts itself: %s", (unsigned long long)r, why); return SPSP_ERR_ARG; }
        if (rec.listed == 0) { ++none; none_bases += rec.length; continue; }
        ++best[h[0].reference]; bases[h[0].reference] += rec.length; keys[h[0].reference] += h[0].shared;
        for (uint32_t i = 0; i < rec.listed; ++i) ++listed[h[i].reference];
    }
    std::string out = "reference,records_best,bases_best,keys_best,records_listed\n";
    for (uint32_t j = 0; j < n_ref; ++j) {
        out += ref_names[j]; out += ',';
        out += std::to_string(best[j]); out += ',';
        out += std::to_string(bases[j]); out += ',';
        out += std::to_string(keys[j]); out += ',';
        out += std::to_string(listed[j]); out += '\n';
    }
    out += "unclassified," + std::to_string(none) + ',' + std::to_string(none_bases) + ",0,0\n";
    return text_out(out, text, len);
}

// ------------------------------------------------------------------------------------------------ taxonomy
// a lineage file: one line per reference, names from below the root down, joined by ';'; a node is a path
int spsp_taxonomy_lineages_host(const char* text, uint64_t len, uint32_t n_ref, uint32_t* ref_node, uint32_t** parent, uint32_t** depth, uint32_t** size,
                                char** names, uint64_t* names_len, uint32_t* n_nodes) {
    using namespace spsp;
    if (parent) *parent = nullptr;
    if (depth) *depth = nullptr;
    if (size) *size = nullptr;
    if (names) *names = nullptr;
    if (names_len) *names_len = 0;
    if (n_nodes) *n_nodes = 0;
    if ((!text && len) || !ref_node || !n_nodes) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_ref == 0 || n_ref > 65535) { set_error("a classification index takes 1 .. 65535 references (n = %u)", n_ref); return SPSP_ERR_ARG; }
    // the trie in order of appearance: node 0 is the root
    struct Node { uint32_t parent; std::string name; std::vector<uint32_t> kids; std::unordered_map<std::string, uint32_t> by_name; };
    std::vector<Node> trie(1);
    trie[0].parent = 0; trie[0].name = "root";
    std::vector<uint32_t> at(n_ref, 0);
    uint64_t line = 0, pos = 0;
    while (pos < len) {
        uint64_t end = pos;
        while (end < len && text[end] != '\n') ++end;
        uint64_t stop = end;
        if (stop > pos && text[stop - 1] == '\r') --stop;  // ("\r\n" is tolerated)
        ++line;
        const unsigned long long ln = (unsigned long long)line;
        if (line > n_ref) { set_error("lineages: line %llu: more lines than the %u references", ln, n_ref); return SPSP_ERR_FORMAT; }
        uint64_t a = pos, z = stop;
        while (a < z && (text[a] == ' ' || text[a] == '\t')) ++a;
        while (z > a && (text[z - 1] == ' ' || text[z - 1] == '\t')) --z;
        uint32_t cur = 0, count = 0;
        for (uint64_t s0 = a; a < z;) {                    // (an empty line: the reference sits at the root)
            uint64_t e = s0;
            while (e < z && text[e] != ';') ++e;
            uint64_t na = s0, nz = e;
            while (na < nz && (text[na] == ' ' || text[na] == '\t')) ++na;
            while (nz > na && (text[nz - 1] == ' ' || text[nz - 1] == '\t')) --nz;
            if (na == nz) { set_error("lineages: line %llu: an empty name", ln); return SPSP_ERR_FORMAT; }
            for (uint64_t q = na; q < nz; ++q) {
                const unsigned char c = (unsigned char)text[q];
                if (c == ',' || c == '"' || c < 0x20 || c == 0x7f) {
                    set_error("lineages: line %llu: a name holds ',', '\"' or a control character (byte 0x%02x)", ln, (unsigned)c);
                    return SPSP_ERR_FORMAT;
                }
            }
            if (++count > kTxMaxDepth) { set_error("lineages: line %llu: more than %u names", ln, kTxMaxDepth); return SPSP_ERR_FORMAT; }
            const std::string name(text + na, (size_t)(nz - na));
            const auto it = trie[cur].by_name.find(name);
            if (it != trie[cur].by_name.end()) cur = it->second;
            else {
                if (trie.size() >= kTxMaxNodes) { set_error("lineages: line %llu: more than %u nodes", ln, kTxMaxNodes); return SPSP_ERR_FORMAT; }
                const uint32_t id = (uint32_t)trie.size();
                trie[cur].by_name.emplace(name, id);
                trie[cur].kids.push_back(id);
                trie.emplace_back();
                trie.back().parent = cur; trie.back().name = name;
                cur = id;
            }
            if (e == z) break;
            s0 = e + 1;                                    // (a ';' at the line's end: one more, empty, name)
        }
        at[line - 1] = cur;
        pos = end + 1;                                     // (the final newline is optional: nothing behind it is no line)
    }
    if (line != n_ref) {
        set_error("lineages: line %llu: the file ends after %llu line(s), %u references are listed", (unsigned long long)(line + 1), (unsigned long long)line, n_ref);
        return SPSP_ERR_FORMAT;
    }
    // preorder numbers, children in order of first appearance
    const uint32_t T = (uint32_t)trie.size();
    std::vector<uint32_t> number(T, 0), order;
    order.reserve(T);
    std::vector<std::pair<uint32_t, uint32_t>> stack{{0u, 0u}};
    order.push_back(0);
    while (!stack.empty()) {
        auto& top = stack.back();
        if (top.second == trie[top.first].kids.size()) { stack.pop_back(); continue; }
        const uint32_t kid = trie[top.first].kids[top.second++];
        number[kid] = (uint32_t)order.size();
        order.push_back(kid);
        stack.push_back({kid, 0u});
    }
    uint32_t* arr[3] = {nullptr, nullptr, nullptr};
    for (uint32_t*& p : arr)
        if (!(p = (uint32_t*)malloc((size_t)T * 4))) { for (uint32_t* q : arr) free(q); set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    std::string blob;
    for (uint32_t t = 0; t < T; ++t) {
        const Node& nd = trie[order[t]];
        arr[0][t] = number[nd.parent];
        arr[1][t] = t ? arr[1][arr[0][t]] + 1u : 0u;
        arr[2][t] = 1u;
        blob.append(nd.name); blob.push_back('\0');
    }
    for (uint32_t t = T - 1; t >= 1; --t) arr[2][arr[0][t]] += arr[2][t];
    for (uint32_t j = 0; j < n_ref; ++j) ref_node[j] = number[at[j]];
    if (names) {
        uint64_t l = 0;
        const int rc = text_out(blob, names, &l);
        if (rc) { for (uint32_t* q : arr) free(q); return rc; }
        if (names_len) *names_len = l;
    }
    if (parent) *parent = arr[0]; else free(arr[0]);
    if (depth) *depth = arr[1]; else free(arr[1]);
    if (size) *size = arr[2]; else free(arr[2]);
    *n_nodes = T;
    return SPSP_OK;
}

// the tree's depths and subtree sizes from its parents, or why the arrays are no preorder tree
static int taxonomy_tree(const uint32_t* parent, uint32_t T, std::vector<uint32_t>* depth, std::vector<uint32_t>* size) {
    using namespace spsp;
    if (!parent) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (T == 0 || T > kTxMaxNodes) { set_error("a taxonomy takes 1 .. %u nodes (T = %u)", kTxMaxNodes, T); return SPSP_ERR_ARG; }
    if (parent[0] != 0) { set_error("taxonomy: node 0 is the root: its parent is 0, not %u", parent[0]); return SPSP_ERR_ARG; }
    depth->assign(T, 0);
    for (uint32_t t = 1; t < T; ++t) {
        if (parent[t] >= t) { set_error("taxonomy: node %u has parent %u: a parent comes before its children", t, parent[t]); return SPSP_ERR_ARG; }
        (*depth)[t] = (*depth)[parent[t]] + 1u;
        if ((*depth)[t] > kTxMaxDepth) { set_error("taxonomy: node %u is deeper than %u", t, kTxMaxDepth); return SPSP_ERR_ARG; }
        uint32_t a = t - 1u;                               // preorder: the parent is the node in front or one of its ancestors
        while (a != parent[t] && a != 0u) a = parent[a];
        if (a != parent[t]) { set_error("taxonomy: node %u is not numbered in preorder: its parent %u is no ancestor of node %u", t, parent[t], t - 1u); return SPSP_ERR_ARG; }
    }
    if (size) {
        size->assign(T, 1);
        for (uint32_t t = T - 1; t >= 1; --t) (*size)[parent[t]] += (*size)[t];
    }
    return SPSP_OK;
}

int spsp_taxonomy_check_host(const uint32_t* parent, uint32_t n_nodes, const uint32_t* ref_node, uint32_t n_ref) {
    using namespace spsp;
    if (!parent || !ref_node) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_ref == 0 || n_ref > 65535) { set_error("a classification index takes 1 .. 65535 references (n = %u)", n_ref); return SPSP_ERR_ARG; }
    std::vector<uint32_t> depth;
    if (const int rc = taxonomy_tree(parent, n_nodes, &depth, nullptr)) return rc;
    for (uint32_t j = 0; j < n_ref; ++j)
        if (ref_node[j] >= n_nodes) { set_error("taxonomy: reference %u sits at node %u, there are %u nodes", j, ref_node[j], n_nodes); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

// the cuts of spsp_taxonomy.hip: the constants of spsp_internal.h
int spsp_taxonomy_plan_host(uint32_t n_nodes, uint32_t* small_hits, uint32_t* lds_nodes, uint32_t* counters_in_lds, uint32_t* list_cut) {
    using namespace spsp;
    if (n_nodes == 0 || n_nodes > kTxMaxNodes) { set_error("a taxonomy takes 1 .. %u nodes (T = %u)", kTxMaxNodes, n_nodes); return SPSP_ERR_ARG; }
    if (small_hits) *small_hits = kTxSmallHits;
    if (lds_nodes) *lds_nodes = kTxLdsNodes;
    if (counters_in_lds) *counters_in_lds = n_nodes <= kTxLdsNodes ? 1u : 0u;
    if (list_cut) *list_cut = kTxListCut;
    return SPSP_OK;
}

// a record's row that cannot be a taxonomy call's: why, or null
static const char* taxonomy_row_wrong(const spsp_taxonomy_record& r, uint32_t T, const std::vector<uint32_t>& size) {
    if (r.hit_keys > r.keys) return "more hit keys than keys";
    if (r.clade > r.hit_keys) return "a clade of more keys than the record has hit keys";
    if (r.direct > r.clade) return "more keys at the node than in its clade";
    if (r.score > r.hit_keys) return "a score above the hit keys";
    if (r.node != SPSP_TAXONOMY_NONE && r.node >= T) return "a node outside the tree";
    if (r.node != SPSP_TAXONOMY_NONE && !(r.node <= r.start && r.start - r.node < size[r.node])) return "a node that is no ancestor of the start";
    if (r.winners == 0 && r.hit_keys > 0) return "hit keys without a winner";
    return nullptr;
}

static void taxonomy_lineage(const uint32_t* parent, const char* const* node_names, uint32_t t, std::string* out) {
    uint32_t way[spsp::kTxMaxDepth + 1], n = 0;
    for (; t != 0u; t = parent[t]) way[n++] = t;           // (depth <= 32: the tree was checked)
    out->clear();
    while (n) { *out += node_names[way[--n]]; if (n) *out += ';'; }
}

int spsp_taxonomy_csv_host(const spsp_taxonomy_record* records, uint64_t n_records, const char* const* record_names, const uint32_t* parent,
                           uint32_t n_nodes, const char* const* node_names, int precision, char** text, uint64_t* len) {
    if (!text || !len || !node_names || (n_records && (!records || !record_names))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::vector<uint32_t> depth, size;
    if (const int rc = taxonomy_tree(parent, n_nodes, &depth, &size)) return rc;
    std::string out = "record,name,length,keys,hit_keys,taxon,depth,lineage,score,clade,direct,f_clade,winners\n", lineage;
    char num[64];
    for (uint64_t r = 0; r < n_records; ++r) {
        const spsp_taxonomy_record& rec = records[r];
        if (const char* why = taxonomy_row_wrong(rec, n_nodes, size)) { set_error("taxonomy record %llu contradicts itself: %s", (unsigned long long)r, why); return SPSP_ERR_ARG; }
        out += std::to_string(r); out += ',';
        out += record_names[r]; out += ',';
        out += std::to_string(rec.length); out += ',';
        out += std::to_string(rec.keys); out += ',';
        out += std::to_string(rec.hit_keys); out += ',';
        const bool called = rec.node != SPSP_TAXONOMY_NONE;
        if (called) {
            taxonomy_lineage(parent, node_names, rec.node, &lineage);
            out += std::to_string(rec.node); out += ',';
            out += std::to_string(depth[rec.node]); out += ',';
            out += lineage; out += ',';
        } else out += ",,,";
        out += std::to_string(rec.score); out += ',';
        out += std::to_string(rec.clade); out += ',';
        out += std::to_string(rec.direct); out += ',';
        out.append(num, format_g(num, sizeof num, precision, called && rec.keys ? (double)rec.clade / (double)rec.keys : 0.0)); out += ',';
        out += std::to_string(rec.winners); out += '\n';
    }
    return text_out(out, text, len);
}

int spsp_taxonomy_report_csv_host(const spsp_taxonomy_record* records, uint64_t n_records, const uint32_t* parent, uint32_t n_nodes,
                                  const char* const* node_names, const uint32_t* ref_node, uint32_t n_ref, char** text, uint64_t* len) {
    if (!text || !len || !node_names || (n_records && !records)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (const int rc = spsp_taxonomy_check_host(parent, n_nodes, ref_node, n_ref)) return rc;
    std::vector<uint32_t> depth, size;
    if (const int rc = taxonomy_tree(parent, n_nodes, &depth, &size)) return rc;
    const uint32_t T = n_nodes;
    std::vector<uint64_t> refs(T, 0), rec_direct(T, 0), rec_clade(T, 0), base_direct(T, 0), base_clade(T, 0);
    uint64_t none = 0, none_bases = 0;
    for (uint32_t j = 0; j < n_ref; ++j) ++refs[ref_node[j]];
    for (uint64_t r = 0; r < n_records; ++r) {
        const spsp_taxonomy_record& rec = records[r];
        if (const char* why = taxonomy_row_wrong(rec, T, size)) { set_error("taxonomy record %llu contradicts itself: %s", (unsigned long long)r, why); return SPSP_ERR_ARG; }
        if (rec.node == SPSP_TAXONOMY_NONE) { ++none; none_bases += rec.length; continue; }
        ++rec_direct[rec.node]; base_direct[rec.node] += rec.length;
    }
    rec_clade = rec_direct; base_clade = base_direct;
    for (uint32_t t = T - 1; t >= 1; --t) { rec_clade[parent[t]] += rec_clade[t]; base_clade[parent[t]] += base_clade[t]; }
    std::string out = "taxon,depth,name,lineage,references,records_clade,records_direct,bases_clade,bases_direct\n", lineage;
    for (uint32_t t = 0; t < T; ++t) {
        taxonomy_lineage(parent, node_names, t, &lineage);
        out += std::to_string(t); out += ',';
        out += std::to_string(depth[t]); out += ',';
        out += node_names[t]; out += ',';
        out += lineage; out += ',';
        out += std::to_string(refs[t]); out += ',';
        out += std::to_string(rec_clade[t]); out += ',';
        out += std::to_string(rec_direct[t]); out += ',';
        out += std::to_string(base_clade[t]); out += ',';
        out += std::to_string(base_direct[t]); out += '\n';
    }
    out += ",,unclassified,,0," + std::to_string(none) + ',' + std::to_string(none) + ',' + std::to_string(none_bases) + ',' + std::to_string(none_bases) + '\n';
    return text_out(out, text, len);
}

// ------------------------------------------------------------------------------------------------ depth
int spsp_depth_plan_host(uint32_t* bins) {
    if (!bins) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *bins = spsp::kDpBins;
    return SPSP_OK;
}

// five numbers that cannot be the statistics of `found` counts: why, or null
static const char* depth_five_wrong(uint32_t found, uint64_t sum, uint32_t median, uint32_t max) {
    if (median > max) return "a median above the maximum";
    if (max > sum) return "a maximum above the sum";
    if (found == 0) return sum || max || median ? "nothing found, and a sum, maximum or median all the same" : nullptr;
    if (median == 0) return "keys found, and a median of 0";
    if (sum < found || sum > (uint64_t)found * max) return "a sum outside found .. found * max";
    return nullptr;
}

static const char* depth_row_wrong(const spsp_depth_row& r) {
    if (r.found > r.keys) return "more keys found than keys";
    if (r.unique_keys > r.keys) return "more unique keys than keys";
    if (r.unique_found > r.found || r.unique_found > r.unique_keys) return "more unique keys found than min(found, unique_keys)";
    if (const char* why = depth_five_wrong(r.found, r.sum, r.median, r.max)) return why;
    if (const char* why = depth_five_wrong(r.unique_found, r.unique_sum, r.unique_median, r.unique_max)) return why;
    if (r.unique_sum > r.sum) return "a unique sum above the sum";
    return nullptr;
}

int spsp_depth_csv_host(const spsp_depth_row* rows, const char* const* names, uint32_t n_ref, int precision, char** text, uint64_t* len) {
    if (!text || !len || (n_ref && (!rows || !names))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::string out = "reference,keys,found,f_found,median,mean,max,unique_keys,unique_found,f_unique_found,unique_median,unique_mean,unique_max\n";
    char num[64];
    for (uint32_t j = 0; j < n_ref; ++j) {
        const spsp_depth_row& r = rows[j];
        if (const char* why = depth_row_wrong(r)) { set_error("depth row of reference %u contradicts itself: %s", j, why); return SPSP_ERR_ARG; }
        out += names[j];
        const uint32_t keys[2] = {r.keys, r.unique_keys}, found[2] = {r.found, r.unique_found}, median[2] = {r.median, r.unique_median}, max[2] = {r.max, r.unique_max};
        const uint64_t sum[2] = {r.sum, r.unique_sum};
        for (int u = 0; u < 2; ++u) {
            out += ','; out += std::to_string(keys[u]);
            out += ','; out += std::to_string(found[u]);
            out += ','; out.append(num, format_g(num, sizeof num, precision, keys[u] ? (double)found[u] / (double)keys[u] : 0.0));
            out += ','; out += std::to_string(median[u]);
            out += ','; out.append(num, format_g(num, sizeof num, precision, found[u] ? (double)sum[u] / (double)found[u] : 0.0));
            out += ','; out += std::to_string(max[u]);
        }
        out += '\n';
    }
    return text_out(out, text, len);
}

// ------------------------------------------------------------------------------------------------ profile
// a row that cannot be round `rank`'s behind `before` (null for the first): why, or null.  left: |A| in front of the round
static const char* profile_row_wrong(const spsp_profile_row& r, const spsp_profile_row* before, uint32_t left, uint32_t n_ref) {
    if (r.reference >= n_ref) return "a reference the index does not have";
    if (r.assigned == 0) return "no key assigned";
    if (r.assigned > r.found) return "more keys assigned than found";
    if (r.found > r.keys) return "more keys found than keys";
    if (before && r.assigned > before->assigned) return "more keys assigned than in the round before";
    if (r.assigned > left || r.remaining != left - r.assigned) return "remaining is not what the round before left, less the keys assigned";
    if (r.median == 0 || r.median > r.max) return "a median outside 1 .. max";
    if (r.sum < r.assigned || r.sum > (uint64_t)r.assigned * r.max) return "a sum outside assigned .. assigned * max";
    return nullptr;
}

int spsp_profile_csv_host(const spsp_profile_row* rows, uint64_t n_rows, const spsp_profile_totals* totals, const char* const* names, uint32_t n_ref,
                          int precision, char** text, uint64_t* len) {
    if (!text || !len || !totals || (n_rows && (!rows || !names))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_rows > n_ref) {
        set_error("profile: %llu rows for %u references (rank %u names a reference twice)", (unsigned long long)n_rows, n_ref, n_ref + 1);
        return SPSP_ERR_ARG;
    }
    std::string out = "rank,reference,keys,found,f_found,assigned,f_assigned,median,mean,max,f_weighted,remaining\n";
    std::vector<uint8_t> seen(n_ref, 0);
    char num[64];
    uint32_t left = totals->found_keys;
    for (uint64_t i = 0; i < n_rows; ++i) {
        const spsp_profile_row& r = rows[i];
        const char* why = profile_row_wrong(r, i ? &rows[i - 1] : nullptr, left, n_ref);
        if (!why && seen[r.reference]) why = "a reference named before";
        if (why) { set_error("profile row of rank %llu contradicts the rule: %s", (unsigned long long)(i + 1), why); return SPSP_ERR_ARG; }
        seen[r.reference] = 1;
        left = r.remaining;
        out += std::to_string(i + 1); out += ',';
        out += names[r.reference];
        out += ','; out += std::to_string(r.keys);
        out += ','; out += std::to_string(r.found);
        out += ','; out.append(num, format_g(num, sizeof num, precision, r.keys ? (double)r.found / (double)r.keys : 0.0));
        out += ','; out += std::to_string(r.assigned);
        out += ','; out.append(num, format_g(num, sizeof num, precision, totals->found_keys ? (double)r.assigned / (double)totals->found_keys : 0.0));
        out += ','; out += std::to_string(r.median);
        out += ','; out.append(num, format_g(num, sizeof num, precision, r.assigned ? (double)r.sum / (double)r.assigned : 0.0));
        out += ','; out += std::to_string(r.max);
        out += ','; out.append(num, format_g(num, sizeof num, precision, totals->found_sum ? (double)r.sum / (double)totals->found_sum : 0.0));
        out += ','; out += std::to_string(r.remaining);
        out += '\n';
    }
    return text_out(out, text, len);
}

// ------------------------------------------------------------------------------------------------ the linkage tree
int spsp_tree_cut_host(const spsp_tree_row* rows, uint64_t n_rows, uint32_t n, const uint64_t* card, int metric, uint32_t floor_num, uint32_t floor_den,
                       uint32_t num, uint32_t den, uint32_t* cluster, uint64_t* n_clusters) {
    if (!cluster || !n_clusters || !card || (n_rows && !rows)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *n_clusters = 0;
    int rc;
    if ((rc = tree_check_metric(metric))) return rc;
    if (n == 0 || n > 65535) { set_error("a tree is over 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (floor_den == 0 || floor_num > floor_den || floor_den > 1000000u || den == 0 || num > den || den > 1000000u) {
        set_error("tree cut %u / %u at floor %u / %u: both need 0 <= num <= den, 1 <= den <= 1000000", num, den, floor_num, floor_den);
        return SPSP_ERR_ARG;
    }
    if ((uint64_t)num * floor_den < (uint64_t)floor_num * den) {
        set_error("tree cut %u / %u is below the floor %u / %u the tree was built at", num, den, floor_num, floor_den);
        return SPSP_ERR_ARG;
    }
    if ((rc = tree_check_rows(rows, n_rows, n))) return rc;
    const uint64_t u_max = num ? ~0ull / num : ~0ull;      // the link test's guard
    TreeSets sets(n);
    for (uint64_t r = 0; r < n_rows; ++r) {
        const uint64_t x = rows[r].shared, u = tree_under(metric, card, rows[r].a, rows[r].b, x);
        if (!(x >= 1 && u <= u_max && (u128)x * den >= (u128)num * u)) continue;
        const uint32_t ra = sets.find(rows[r].a), rb = sets.find(rows[r].b);
        if (ra != rb) sets.unite(ra, rb);
    }
    uint32_t count = 0;
    for (uint32_t i = 0; i < n; ++i) {                     // a root is its set's first-listed member: numbered before its members are
        const uint32_t r = sets.find(i);
        cluster[i] = r == i ? count++ : cluster[r];
    }
    *n_clusters = count;
    return SPSP_OK;
}

int spsp_tree_csv_host(const spsp_tree_row* rows, uint64_t n_rows, const char* const* names, uint32_t n, const uint64_t* card, int metric, int precision,
                       char** text, uint64_t* len) {
    if (!text || !len || (n_rows && (!rows || !names || !card))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = tree_check_metric(metric)) || (rc = tree_check_rows(rows, n_rows, std::max(n, 1u)))) return rc;
    std::string out = "step,a,b,shared,keys_a,keys_b,score,size,clusters\n";
    char num[64];
    for (uint64_t r = 0; r < n_rows; ++r) {
        const spsp_tree_row& t = rows[r];
        const uint64_t under = tree_under(metric, card, t.a, t.b, t.shared);
        out += std::to_string(r + 1); out += ',';
        out += names[t.a]; out += ',';
        out += names[t.b]; out += ',';
        out += std::to_string(t.shared); out += ',';
        out += std::to_string(card[t.a]); out += ',';
        out += std::to_string(card[t.b]); out += ',';
        out.append(num, format_g(num, sizeof num, precision, (double)t.shared / (double)under)); out += ',';   // (printed only: the integer order has decided)
        out += std::to_string(t.size); out += ',';
        out += std::to_string(n - (r + 1)); out += '\n';
    }
    return text_out(out, text, len);
}

int spsp_tree_newick_host(const spsp_tree_row* rows, uint64_t n_rows, const char* const* names, uint32_t n, const uint64_t* card, int metric, int precision,
                          char** text, uint64_t* len) {
    if (!text || !len || !names || (n_rows && (!rows || !card))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = tree_check_metric(metric))) return rc;
    if (n == 0 || n > 65535) { set_error("a tree is over 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if ((rc = tree_check_rows(rows, n_rows, n))) return rc;
    // nodes: 0 .. n-1 the leaves, then one per row, then one per join of two components that never merged: 2 n - 1 in all
    const uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> left(2 * (size_t)n - 1, kNone), right(2 * (size_t)n - 1, kNone), above(2 * (size_t)n - 1, kNone);
    std::vector<double> height(2 * (size_t)n - 1, 0.0);
    std::vector<uint32_t> node_of(n);                      // a set's root sketch (its first-listed member) -> the node on top of the set
    for (uint32_t i = 0; i < n; ++i) node_of[i] = i;
    TreeSets sets(n);
    uint32_t nodes = n;
    auto join = [&](uint32_t ra, uint32_t rb, double h) {  // two roots: the set with the smaller first member comes first
        if (ra > rb) std::swap(ra, rb);
        left[nodes] = node_of[ra]; right[nodes] = node_of[rb]; height[nodes] = h;
        above[node_of[ra]] = nodes; above[node_of[rb]] = nodes;
        node_of[sets.unite(ra, rb)] = nodes++;
    };
    for (uint64_t r = 0; r < n_rows; ++r) {
        const uint32_t ra = sets.find(rows[r].a), rb = sets.find(rows[r].b);
        if (ra == rb) { set_error("tree row %llu joins two sketches that are joined already", (unsigned long long)r); return SPSP_ERR_ARG; }
        join(ra, rb, 1.0 - (double)rows[r].shared / (double)tree_under(metric, card, rows[r].a, rows[r].b, rows[r].shared));
    }
    for (uint32_t i = 1; i < n; ++i)                       // what never merged: at height 1, one after another (sketch 0 is in the first)
        if (sets.find(i) == i) join(0, i, 1.0);
    // written by an explicit stack (a path of 65 535 sketches is 65 534 levels deep): a node, or what follows a node
    enum : uint32_t { kOpen = 0, kComma = 1, kClose = 2, kLength = 3 };
    struct Item { uint32_t node, what; };
    std::vector<Item> stack;
    std::string out;
    char num[64];
    stack.push_back(Item{nodes - 1, kOpen});
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        if (it.what == kComma) { out += ','; continue; }
        if (it.what == kClose) { out += ')'; continue; }
        if (it.what == kLength) {
            out += ':';
            out.append(num, format_g(num, sizeof num, precision, height[above[it.node]] - height[it.node]));
            continue;
        }
        if (it.node < n) { newick_leaf(out, names[it.node]); continue; }
        out += '(';
        stack.push_back(Item{0, kClose});
        stack.push_back(Item{right[it.node], kLength});
        stack.push_back(Item{right[it.node], kOpen});
        stack.push_back(Item{0, kComma});
        stack.push_back(Item{left[it.node], kLength});
        stack.push_back(Item{left[it.node], kOpen});
    }
    out += ";\n";
    return text_out(out, text, len);
}

int spsp_compare_files_rate(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, double min_threshold,
                            const char* out_prefix, int chatter, double rate) {
    return compare_files_impl(ctx, paths, n, n_query, precision, min_threshold, out_prefix, clamp_chatter(chatter), rate);
}
int spsp_compare_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision,
                       double min_threshold, const char* out_prefix) {
    return spsp_compare_files_rate(ctx, paths, n, n_query, precision, min_threshold, out_prefix, 0, SPSP_RATE_AS_IS);
}
int spsp_compare_files_chatty(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision,
                              double min_threshold, const char* out_prefix, int all_versus_all) {
    return spsp_compare_files_rate(ctx, paths, n, n_query, precision, min_threshold, out_prefix, all_versus_all ? 1 : 2, SPSP_RATE_AS_IS);
}

int spsp_compare_files_multi(const int* devices, uint32_t n_dev, const char* const* paths, uint32_t n, uint32_t n_query, int precision,
                             double min_threshold, const char* out_prefix, int chatter, spsp_stage_times* times) {
    return spsp_compare_files_multi_rate(devices, n_dev, paths, n, n_query, precision, min_threshold, out_prefix, chatter, times, SPSP_RATE_AS_IS);
}

int spsp_compare_files_multi_rate(const int* devices, uint32_t n_dev, const char* const* paths, uint32_t n, uint32_t n_query, int precision,
                                  double min_threshold, const char* out_prefix, int chatter, spsp_stage_times* times, double rate) {
    if (!devices || n_dev == 0 || n_dev > 64 || !paths || !out_prefix) { set_error("1..64 devices, file list and output prefix"); return SPSP_ERR_ARG; }
    std::vector<spsp_ctx*> ctxs;
    int rc = SPSP_OK;
    if (getenv("SPSP_DEBUG_MULTI_TRACE")) {                   // which devices a CLI run chose (tests/test_multi_device.py)
        std::string devs;
        for (uint32_t d = 0; d < n_dev; ++d) devs += (d ? "," : "") + std::to_string(devices[d]);
        fprintf(stderr, "spsp multi: %u contexts on devices %s, %u sketches\n", n_dev, devs.c_str(), n);
    }
    for (uint32_t d = 0; d < n_dev && !rc; ++d) {
        spsp_ctx* c = nullptr;
        rc = spsp_create(devices[d], nullptr, &c);
        if (!rc) ctxs.push_back(c);
    }
    if (!rc) rc = compare_files_impl(ctxs[0], paths, n, n_query, precision, min_threshold, out_prefix, clamp_chatter(chatter), rate, ctxs.data(), (uint32_t)ctxs.size());
    if (!rc && times) *times = ctxs[0]->stages;
    const std::string err = rc ? spsp_last_error() : "";
    for (spsp_ctx* c : ctxs) spsp_destroy(c);
    if (rc) set_error("%s", err.c_str());
    return rc;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------- extract
// The host forms of the extraction, plain loops straight from the rule of include/spsp.h ("extract"): what the device pass is held
// against, and what turns a word and a pass's rows into keep flags.

extern "C" int spsp_extract_plan_host(uint32_t* tile_bytes, uint32_t* stretch_bytes) {
    if (tile_bytes) *tile_bytes = spsp::kExTile;
    if (stretch_bytes) *stretch_bytes = spsp::kExStretch;
    return SPSP_OK;
}

extern "C" int spsp_union_plan_host(uint32_t* threads, uint32_t* tile) {
    if (threads) *threads = spsp::kUnThreads;
    if (tile) *tile = spsp::kUnTile;
    return SPSP_OK;
}

// the naming rule of paired records (include/spsp.h): mate 1's word less one trailing "/1" against mate 2's less one trailing "/2"
extern "C" int spsp_pairs_names_host(const char* const* names1, const char* const* names2, uint64_t n, char** common, uint64_t* bad) {
    using namespace spsp;
    if (common) *common = nullptr;
    if (bad) *bad = n;
    if (!bad || (n && (!names1 || !names2))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::string blob;
    for (uint64_t p = 0; p < n; ++p) {
        if (!names1[p] || !names2[p]) { set_error("NULL argument"); return SPSP_ERR_ARG; }
        size_t l1 = strlen(names1[p]), l2 = strlen(names2[p]);
        if (l1 >= 2 && names1[p][l1 - 2] == '/' && names1[p][l1 - 1] == '1') l1 -= 2;
        if (l2 >= 2 && names2[p][l2 - 2] == '/' && names2[p][l2 - 1] == '2') l2 -= 2;
        if (l1 != l2 || memcmp(names1[p], names2[p], l1) != 0) {
            *bad = p;
            set_error("pair %llu: the mates' names differ ('%.200s' and '%.200s'): are the two files in step?", (unsigned long long)p, names1[p], names2[p]);
            return SPSP_ERR_FORMAT;
        }
        if (common) { blob.append(names1[p], l1); blob.push_back('\0'); }
    }
    if (common) {
        *common = (char*)malloc(blob.size() ? blob.size() : 1);
        if (!*common) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
        memcpy(*common, blob.data(), blob.size());
    }
    return SPSP_OK;
}

extern "C" int spsp_records_extents_host(const uint8_t* text, uint64_t n, uint64_t** begin, uint32_t* n_rec) {
    using namespace spsp;
    if (begin) *begin = nullptr;
    if (n_rec) *n_rec = 0;
    if (!begin || !n_rec || (n && !text)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::vector<uint64_t> b;
    if (n > 0 && text[0] == '@') {
        uint64_t end = n;
        while (end && (text[end - 1] == '\n' || text[end - 1] == '\r')) --end;   // the content: the text less its blank tail
        uint64_t lines = 1;
        b.push_back(0);
        for (uint64_t p = 0; p < end; ++p)
            if (text[p] == '\n' && lines++ % 4 == 0) b.push_back(p + 1);         // line `lines` begins behind this newline
        uint64_t last = end;                               // the last record ends behind the newline of its fourth line, where it has one
        for (uint64_t p = end; p < n; ++p)
            if (text[p] == '\n') { last = p + 1; break; }
        if (lines % 4 == 3 && last > end && last < n) {    // an empty quality line given by the blank tail: the ingest's empty read
            ++lines;
            const uint64_t from = last;
            last = n;
            for (uint64_t p = from; p < n; ++p)
                if (text[p] == '\n') { last = p + 1; break; }
        }
        if (lines % 4 != 0) { set_error("FASTQ: the content has %llu line(s), which is not a multiple of four", (unsigned long long)lines); return SPSP_ERR_FORMAT; }
        b.push_back(last);
    } else {
        b.push_back(0);                                    // line 0 is a header whatever it holds
        for (uint64_t p = 1; p < n; ++p)
            if (text[p - 1] == '\n' && (text[p] == '>' || text[p] == 0xFFu)) b.push_back(p);
        b.push_back(n);
    }
    if (b.size() - 1 > 0xfffffff0ull) { set_error("too many records for one call"); return SPSP_ERR_OVERFLOW; }
    *begin = (uint64_t*)malloc(b.size() * 8);
    if (!*begin) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    memcpy(*begin, b.data(), b.size() * 8);
    *n_rec = (uint32_t)(b.size() - 1);
    return SPSP_OK;
}

extern "C" int spsp_records_extract_host(const uint8_t* text, uint64_t n, const uint64_t* begin, uint32_t n_rec, const uint8_t* keep, uint8_t** out,
                                         uint64_t* n_out, uint64_t* n_kept) {
    using namespace spsp;
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (n_kept) *n_kept = 0;
    if (!out || !n_out || !n_kept || !begin || (n && !text) || (n_rec && !keep)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    uint64_t bytes = 0, kept = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        if (begin[r] > begin[r + 1] || begin[r + 1] > n) { set_error("extract: begin must not decrease and must end inside the text"); return SPSP_ERR_ARG; }
        if (!keep[r]) continue;
        ++kept;
        bytes += begin[r + 1] - begin[r];
        if (r + 1 == n_rec && begin[r + 1] > begin[r] && text[begin[r + 1] - 1] != '\n') ++bytes;   // (only the last record can lack its newline)
    }
    uint8_t* o = (uint8_t*)malloc(bytes ? bytes : 1);
    if (!o) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint64_t len = begin[r + 1] - begin[r];
        if (!keep[r] || !len) continue;
        memcpy(o + at, text + begin[r], len);
        at += len;
        if (r + 1 == n_rec && o[at - 1] != '\n') o[at++] = '\n';
    }
    *out = o; *n_out = at; *n_kept = kept;
    return SPSP_OK;
}

namespace {

// "<name>=<number>": the number, decimal digits only, as 32 bits
bool extract_word_number(const char* what, const char* name, uint32_t* value) {
    const size_t len = strlen(name);
    if (strncmp(what, name, len) != 0 || what[len] != '=') return false;
    const char* p = what + len + 1;
    if (!*p) return false;
    uint64_t v = 0;
    for (; *p; ++p) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (uint64_t)(*p - '0');
        if (v > 0xffffffffull) return false;
    }
    *value = (uint32_t)v;
    return true;
}

enum ExtractWord { kXwNone = 0, kXwMatched, kXwUnmatched, kXwBest, kXwListed, kXwClassified, kXwUnclassified, kXwTaxon, kXwClade };

ExtractWord extract_word(const char* what, uint32_t* value) {
    *value = 0;
    if (!strcmp(what, "matched")) return kXwMatched;
    if (!strcmp(what, "unmatched")) return kXwUnmatched;
    if (!strcmp(what, "classified")) return kXwClassified;
    if (!strcmp(what, "unclassified")) return kXwUnclassified;
    if (extract_word_number(what, "best", value)) return kXwBest;
    if (extract_word_number(what, "listed", value)) return kXwListed;
    if (extract_word_number(what, "taxon", value)) return kXwTaxon;
    if (extract_word_number(what, "clade", value)) return kXwClade;
    return kXwNone;
}

// the word of a call with classify rows (taxonomy == false) or taxonomy rows, or its refusal
int extract_word_for(const char* what, bool taxonomy, ExtractWord* word, uint32_t* value) {
    using namespace spsp;
    if (!what) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *word = extract_word(what, value);
    if (*word == kXwNone) {
        set_error("extract: '%.64s' names no records (%s)", what,
                  taxonomy ? "with a taxonomy: classified, unclassified, taxon=<t>, clade=<t>" : "matched, unmatched, best=<j>, listed=<j>");
        return SPSP_ERR_ARG;
    }
    const bool taxonomy_word = *word >= kXwClassified;
    if (taxonomy_word != taxonomy) {
        set_error(taxonomy ? "extract: '%.64s' asks classify's rows, these are a taxonomy's (classified, unclassified, taxon=<t>, clade=<t>)"
                           : "extract: '%.64s' asks a taxonomy's rows, these are classify's (matched, unmatched, best=<j>, listed=<j>)", what);
        return SPSP_ERR_ARG;
    }
    return SPSP_OK;
}

}  // namespace

extern "C" int spsp_extract_word_check_host(const char* what, int taxonomy, uint32_t limit) {
    using namespace spsp;
    ExtractWord word; uint32_t v = 0;
    if (const int rc = extract_word_for(what, taxonomy != 0, &word, &v)) return rc;
    if ((word == kXwBest || word == kXwListed) && v >= limit) { set_error("extract: '%.64s': the index has %u reference(s)", what, limit); return SPSP_ERR_ARG; }
    if ((word == kXwTaxon || word == kXwClade) && v >= limit) { set_error("extract: '%.64s': the tree has %u node(s)", what, limit); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

extern "C" int spsp_extract_flags_classify_host(const char* what, const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records,
                                                uint32_t top, uint32_t n_ref, uint8_t* keep) {
    using namespace spsp;
    if (n_records && (!records || !hits || !keep)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (top == 0 || top > kCfMaxTop) { set_error("top must be 1 .. %u (top = %u)", kCfMaxTop, top); return SPSP_ERR_ARG; }
    if (const int rc = spsp_extract_word_check_host(what, 0, n_ref)) return rc;
    ExtractWord word; uint32_t j = 0;
    (void)extract_word_for(what, false, &word, &j);
    for (uint64_t r = 0; r < n_records; ++r) {
        const uint32_t listed = records[r].listed;
        if (listed > top) { set_error("extract: record %llu lists %u matches, top = %u", (unsigned long long)r, listed, top); return SPSP_ERR_ARG; }
        const spsp_classify_hit* h = hits + r * top;
        bool k = false;
        switch (word) {
            case kXwMatched: k = listed >= 1; break;
            case kXwUnmatched: k = listed == 0; break;
            case kXwBest: k = listed >= 1 && h[0].reference == j; break;
            default:
                for (uint32_t i = 0; i < listed; ++i) k = k || h[i].reference == j;
        }
        keep[r] = k ? 1 : 0;
    }
    return SPSP_OK;
}

extern "C" int spsp_extract_flags_taxonomy_host(const char* what, const spsp_taxonomy_record* records, uint64_t n_records, const uint32_t* size,
                                                uint32_t n_nodes, uint8_t* keep) {
    using namespace spsp;
    if (!size || (n_records && (!records || !keep))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_nodes == 0 || n_nodes > kTxMaxNodes) { set_error("a taxonomy takes 1 .. %u nodes (T = %u)", kTxMaxNodes, n_nodes); return SPSP_ERR_ARG; }
    if (const int rc = spsp_extract_word_check_host(what, 1, n_nodes)) return rc;
    ExtractWord word; uint32_t t = 0;
    (void)extract_word_for(what, true, &word, &t);
    for (uint64_t r = 0; r < n_records; ++r) {
        const uint32_t node = records[r].node;
        bool k = false;
        switch (word) {
            case kXwClassified: k = node != SPSP_TAXONOMY_NONE; break;
            case kXwUnclassified: k = node == SPSP_TAXONOMY_NONE; break;
            case kXwTaxon: k = node == t; break;
            default: k = node != SPSP_TAXONOMY_NONE && t <= node && node - t < size[t];   // the preorder range: t <= node < t + size[t]
        }
        keep[r] = k ? 1 : 0;
    }
    return SPSP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- split
// The host forms of the split, plain loops straight from the rule of include/spsp.h ("split"): what the device pass is held
// against, what turns a word and a pass's rows into bins, and the manifest's text.

extern "C" int spsp_split_plan_host(uint32_t* stretch_bytes, uint32_t* record_tile, uint32_t* sort_tile, uint32_t* max_bins) {
    if (stretch_bytes) *stretch_bytes = spsp::kExStretch;
    if (record_tile) *record_tile = spsp::kExRecTile;
    if (sort_tile) *sort_tile = spsp::kRsTile;
    if (max_bins) *max_bins = spsp::kSpMaxBins;
    return SPSP_OK;
}

extern "C" int spsp_records_split_host(const uint8_t* text, uint64_t n, const uint64_t* begin, uint32_t n_rec, const uint32_t* bin, uint32_t n_bins, uint8_t** out,
                                       uint64_t* n_out, uint64_t** bin_off, uint64_t** bin_records) {
    using namespace spsp;
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (bin_off) *bin_off = nullptr;
    if (bin_records) *bin_records = nullptr;
    if (!out || !n_out || !bin_off || !bin_records || !begin || (n && !text) || (n_rec && !bin)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_bins == 0 || n_bins > kSpMaxBins) { set_error("split: n_bins must be 1 .. %u (n_bins = %u)", kSpMaxBins, n_bins); return SPSP_ERR_ARG; }
    std::vector<uint64_t> bytes(n_bins, 0), records(n_bins, 0);
    const auto newline = [&](uint32_t r) { return r + 1 == n_rec && begin[r + 1] > begin[r] && text[begin[r + 1] - 1] != '\n'; };   // (only the last record can lack its newline)
    for (uint32_t r = 0; r < n_rec; ++r) {
        if (begin[r] > begin[r + 1] || begin[r + 1] > n) { set_error("split: begin must not decrease and must end inside the text"); return SPSP_ERR_ARG; }
        if (bin[r] == SPSP_SPLIT_DROP) continue;
        if (bin[r] >= n_bins) { set_error("split: bin[%u] = %u, n_bins = %u", r, bin[r], n_bins); return SPSP_ERR_ARG; }
        ++records[bin[r]];
        bytes[bin[r]] += begin[r + 1] - begin[r] + (newline(r) ? 1 : 0);
    }
    uint64_t* off = (uint64_t*)malloc(((size_t)n_bins + 1) * 8);
    uint64_t* rec = (uint64_t*)malloc((size_t)n_bins * 8);
    uint64_t total = 0;
    for (uint32_t b = 0; b < n_bins && off; ++b) { off[b] = total; total += bytes[b]; }
    uint8_t* o = (uint8_t*)malloc(total ? total : 1);
    if (!off || !rec || !o) { free(off); free(rec); free(o); set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    off[n_bins] = total;
    memcpy(rec, records.data(), (size_t)n_bins * 8);
    std::vector<uint64_t> at(off, off + n_bins);           // where the next record of a bin goes
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint64_t len = begin[r + 1] - begin[r];
        if (bin[r] == SPSP_SPLIT_DROP || !len) continue;
        uint64_t& a = at[bin[r]];
        memcpy(o + a, text + begin[r], len);
        a += len;
        if (newline(r)) o[a++] = '\n';
    }
    *out = o; *n_out = total; *bin_off = off; *bin_records = rec;
    return SPSP_OK;
}

namespace {

enum SplitWord { kSwNone = 0, kSwBest, kSwTaxon, kSwDepth };

// the word of a call with classify rows (taxonomy == false) or taxonomy rows, or its refusal; *d: the depth of depth=<d>
int split_word_for(const char* what, bool taxonomy, SplitWord* word, uint32_t* d) {
    using namespace spsp;
    if (!what) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *d = 0;
    *word = !strcmp(what, "best") ? kSwBest : !strcmp(what, "taxon") ? kSwTaxon : extract_word_number(what, "depth", d) ? kSwDepth : kSwNone;
    if (*word == kSwNone) {
        set_error("split: '%.64s' names no bins (%s)", what, taxonomy ? "with a taxonomy: taxon, depth=<d>" : "best");
        return SPSP_ERR_ARG;
    }
    if ((*word != kSwBest) != taxonomy) {
        set_error(taxonomy ? "split: '%.64s' asks classify's rows, these are a taxonomy's (taxon, depth=<d>)"
                           : "split: '%.64s' asks a taxonomy's rows, these are classify's (best)", what);
        return SPSP_ERR_ARG;
    }
    if (*word == kSwDepth && (*d == 0 || *d > kTxMaxDepth)) { set_error("split: '%.64s': the depth must be 1 .. %u", what, kTxMaxDepth); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

}  // namespace

extern "C" int spsp_split_word_check_host(const char* what, int taxonomy) {
    SplitWord word; uint32_t d = 0;
    return split_word_for(what, taxonomy != 0, &word, &d);
}

extern "C" int spsp_split_bins_classify_host(const char* what, const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records, uint32_t top,
                                             uint32_t n_ref, uint32_t* bin, uint32_t* n_bins) {
    using namespace spsp;
    if (n_bins) *n_bins = 0;
    if (!n_bins || (n_records && (!records || !hits || !bin))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (top == 0 || top > kCfMaxTop) { set_error("top must be 1 .. %u (top = %u)", kCfMaxTop, top); return SPSP_ERR_ARG; }
    if (n_ref == 0 || n_ref > 65535u) { set_error("n_ref must be 1 .. 65535 (n_ref = %u)", n_ref); return SPSP_ERR_ARG; }
    SplitWord word; uint32_t d = 0;
    if (const int rc = split_word_for(what, false, &word, &d)) return rc;
    for (uint64_t r = 0; r < n_records; ++r) {
        const uint32_t listed = records[r].listed;
        if (listed > top) { set_error("split: record %llu lists %u matches, top = %u", (unsigned long long)r, listed, top); return SPSP_ERR_ARG; }
        const uint32_t j = listed ? hits[r * top].reference : n_ref;
        if (j > n_ref || (listed && j == n_ref)) { set_error("split: record %llu names reference %u, the index has %u", (unsigned long long)r, j, n_ref); return SPSP_ERR_ARG; }
        bin[r] = j;
    }
    *n_bins = n_ref + 1;
    return SPSP_OK;
}

extern "C" int spsp_split_bins_taxonomy_host(const char* what, const spsp_taxonomy_record* records, uint64_t n_records, const uint32_t* parent, const uint32_t* depth,
                                             uint32_t n_nodes, uint32_t* bin, uint32_t* n_bins) {
    using namespace spsp;
    if (n_bins) *n_bins = 0;
    if (!n_bins || !parent || !depth || (n_records && (!records || !bin))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_nodes == 0 || n_nodes > kTxMaxNodes) { set_error("a taxonomy takes 1 .. %u nodes (T = %u)", kTxMaxNodes, n_nodes); return SPSP_ERR_ARG; }
    SplitWord word; uint32_t d = 0;
    if (const int rc = split_word_for(what, true, &word, &d)) return rc;
    for (uint64_t r = 0; r < n_records; ++r) {
        uint32_t node = records[r].node;
        if (node == SPSP_TAXONOMY_NONE) { bin[r] = n_nodes; continue; }
        if (node >= n_nodes) { set_error("split: record %llu names node %u, the tree has %u", (unsigned long long)r, node, n_nodes); return SPSP_ERR_ARG; }
        if (word == kSwDepth)
            for (uint32_t steps = 0; depth[node] > d && steps < kTxMaxDepth && parent[node] < node; ++steps) node = parent[node];   // (a tree of the lineages' making ends every climb)
        bin[r] = node;
    }
    *n_bins = n_nodes + 1;
    return SPSP_OK;
}

namespace spsp {
std::string split_file_name(const char* prefix, uint32_t b, uint32_t n_bins, const char* last_name, const char* tag, const char* suffix) {
    return std::string(prefix) + "_split_" + (b + 1 == n_bins ? std::string(last_name) : std::to_string(b)) + tag + suffix;
}
}  // namespace spsp

extern "C" int spsp_split_csv_host(const char* file_prefix, const char* const* names, const char* last_name, uint32_t n_bins, const uint64_t* bin_records,
                                   const uint64_t* bin_off, const char* suffix, const uint64_t* bin_off_mates, const char* suffix_mates, char** text, uint64_t* len) {
    using namespace spsp;
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!text || !len || !file_prefix || !last_name || !bin_records || !bin_off || !suffix || (n_bins > 1 && !names) || (bin_off_mates && !suffix_mates)) {
        set_error("NULL argument");
        return SPSP_ERR_ARG;
    }
    if (n_bins == 0 || n_bins > kSpMaxBins) { set_error("split: n_bins must be 1 .. %u (n_bins = %u)", kSpMaxBins, n_bins); return SPSP_ERR_ARG; }
    std::string s = bin_off_mates ? "bin,name,records,bytes_1,file_1,bytes_2,file_2\n" : "bin,name,records,bytes,file\n";
    for (uint32_t b = 0; b < n_bins; ++b) {
        if (!bin_records[b]) continue;
        const bool last = b + 1 == n_bins;
        if (!last && !names[b]) { set_error("NULL argument"); return SPSP_ERR_ARG; }
        s += last ? std::string(last_name) : std::to_string(b);
        s += ","; s += last ? last_name : names[b];
        s += "," + std::to_string(bin_records[b]) + "," + std::to_string(bin_off[b + 1] - bin_off[b]) + ",";
        s += split_file_name(file_prefix, b, n_bins, last_name, bin_off_mates ? "_1" : "", suffix);
        if (bin_off_mates) s += "," + std::to_string(bin_off_mates[b + 1] - bin_off_mates[b]) + "," + split_file_name(file_prefix, b, n_bins, last_name, "_2", suffix_mates);
        s += "\n";
    }
    *text = (char*)malloc(s.size() + 1);
    if (!*text) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    memcpy(*text, s.c_str(), s.size() + 1);
    *len = s.size();
    return SPSP_OK;
}

// -------------------------------------------------------------------------------------------------------------- windows
// The host forms of the windows pass, plain loops straight from the rule of include/spsp.h ("windows"): the counting rule, the
// expansion the device pass is held against, what turns the windows' calls into segments and mosaic rows, and the two texts.

extern "C" int spsp_windows_plan_host(uint32_t* stretch_bases, uint32_t* stretch_bases_packed, uint32_t* record_tile) {
    if (stretch_bases) *stretch_bases = spsp::kWnStretch;
    if (stretch_bases_packed) *stretch_bases_packed = spsp::kWnStretchPacked;
    if (record_tile) *record_tile = spsp::kWnRecTile;
    return SPSP_OK;
}

namespace {

int windows_width_check(uint32_t k, uint64_t window) {
    using namespace spsp;
    if (k == 0 || window < k || window > kWnMaxWidth) {
        set_error("windows: the width must be k .. %llu (k = %u, width = %llu)", (unsigned long long)kWnMaxWidth, k, (unsigned long long)window);
        return SPSP_ERR_ARG;
    }
    return SPSP_OK;
}

// first_win[0 .. n_rec] and the totals from the offsets; nothing is allocated
int windows_count(const uint64_t* rec_off, uint32_t n_rec, uint32_t k, uint64_t window, uint32_t* first_win, uint64_t* n_windows, uint64_t* n_bases) {
    using namespace spsp;
    if (const int rc = windows_width_check(k, window)) return rc;
    const uint64_t S = window - (k - 1);
    uint64_t wins = 0, bases = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        if (rec_off[r] > rec_off[r + 1]) { set_error("windows: the offsets must not decrease (record %u)", r); return SPSP_ERR_ARG; }
        const uint64_t L = rec_off[r + 1] - rec_off[r], n = wn_count(L, k, S);
        if (first_win) first_win[r] = (uint32_t)wins;
        if (n > kWnMaxWindows || wins + n > kWnMaxWindows) {
            set_error("windows: more than %llu windows (at record %u): a wider window, or fewer records per call", (unsigned long long)kWnMaxWindows, r);
            return SPSP_ERR_OVERFLOW;
        }
        wins += n;
        bases += wn_bases(L, n, k);
    }
    if (first_win) first_win[n_rec] = (uint32_t)wins;
    *n_windows = wins; *n_bases = bases;
    return SPSP_OK;
}

int give_text(const std::string& s, char** text, uint64_t* len) {
    *text = (char*)malloc(s.size() + 1);
    if (!*text) { spsp::set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    memcpy(*text, s.c_str(), s.size() + 1);
    *len = s.size();
    return SPSP_OK;
}

}  // namespace

extern "C" int spsp_records_windows_host(const uint64_t* rec_off, uint32_t n_rec, uint32_t k, uint64_t window, uint32_t* first_win, uint64_t** win_off,
                                         uint64_t* n_windows, uint64_t* n_bases) {
    using namespace spsp;
    if (win_off) *win_off = nullptr;
    if (n_windows) *n_windows = 0;
    if (n_bases) *n_bases = 0;
    if (!rec_off || !first_win || !win_off || !n_windows || !n_bases) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    uint64_t wins = 0, bases = 0;
    if (const int rc = windows_count(rec_off, n_rec, k, window, first_win, &wins, &bases)) return rc;
    uint64_t* off = (uint64_t*)malloc(((size_t)wins + 1) * 8);
    if (!off) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    const uint64_t S = window - (k - 1);
    uint64_t at = 0, w = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint64_t L = rec_off[r + 1] - rec_off[r], n = wn_count(L, k, S);
        for (uint64_t i = 0; i < n; ++i) { off[w++] = at; at += std::min<uint64_t>(i * S + window, L) - i * S; }
    }
    off[wins] = at;
    *win_off = off; *n_windows = wins; *n_bases = bases;
    return SPSP_OK;
}

extern "C" int spsp_windows_expand_host(const uint8_t* bases, const uint64_t* rec_off, uint32_t n_rec, uint32_t k, uint64_t window, uint8_t** out, uint64_t* n_out,
                                        uint32_t* first_win, uint64_t** win_off, uint64_t* n_windows) {
    using namespace spsp;
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!out || !n_out || !rec_off || (n_rec && rec_off[n_rec] && !bases)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    uint64_t total = 0;
    if (const int rc = spsp_records_windows_host(rec_off, n_rec, k, window, first_win, win_off, n_windows, &total)) return rc;
    uint8_t* o = (uint8_t*)malloc(total ? (size_t)total : 1);
    if (!o) { free(*win_off); *win_off = nullptr; *n_windows = 0; set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    const uint64_t S = window - (k - 1);
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint64_t L = rec_off[r + 1] - rec_off[r], n = wn_count(L, k, S);
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t p = i * S; p < std::min<uint64_t>(i * S + window, L); ++p) o[at++] = bases[rec_off[r] + p];
    }
    *out = o; *n_out = total;
    return SPSP_OK;
}

extern "C" int spsp_windows_segments_host(const uint32_t* call, const uint32_t* keys, const uint32_t* hit_keys, const uint32_t* support, const uint32_t* first_win,
                                          const uint64_t* rec_off, uint32_t n_rec, uint32_t k, uint64_t window, uint32_t n_bins, spsp_segment_row** segments,
                                          uint64_t* n_segments, spsp_mosaic_row* mosaic) {
    using namespace spsp;
    if (segments) *segments = nullptr;
    if (n_segments) *n_segments = 0;
    if (!segments || !n_segments || !first_win || !rec_off || (n_rec && (!mosaic || !call || !keys || !hit_keys || !support))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (const int rc = windows_width_check(k, window)) return rc;
    if (n_bins == 0) { set_error("windows: n_bins must be 1 or more"); return SPSP_ERR_ARG; }
    const uint64_t S = window - (k - 1);
    const uint32_t none = n_bins - 1;
    std::vector<spsp_segment_row> segs;
    std::vector<std::pair<uint32_t, uint32_t>> order;      // (call, segment) of one record, to add the segments up per call
    uint64_t expect = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        if (rec_off[r] > rec_off[r + 1]) { set_error("windows: the offsets must not decrease (record %u)", r); return SPSP_ERR_ARG; }
        const uint64_t L = rec_off[r + 1] - rec_off[r], n = wn_count(L, k, S);
        if (first_win[r] != expect || n > kWnMaxWindows - expect || first_win[r + 1] != expect + n) {
            set_error("windows: record %u has %llu window(s) from %llu on by the rule, first_win says %u .. %u", r, (unsigned long long)n, (unsigned long long)expect,
                      first_win[r], first_win[r + 1]);
            return SPSP_ERR_ARG;
        }
        expect += n;
        spsp_mosaic_row m{};
        m.length = L; m.windows = (uint32_t)n; m.major = m.second = SPSP_WINDOWS_ABSENT;
        const size_t seg0 = segs.size();
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t w = first_win[r] + i;
            if (call[w] >= n_bins) { set_error("windows: record %u, window %llu: call %u, n_bins = %u", r, (unsigned long long)i, call[w], n_bins); return SPSP_ERR_ARG; }
            const uint64_t end = i + 1 == n ? L : (i + 1) * S;
            if (segs.size() == seg0 || segs.back().call != call[w]) {
                spsp_segment_row s{};
                s.begin = i * S; s.record = r; s.segment = (uint32_t)(segs.size() - seg0); s.call = call[w];
                segs.push_back(s);
            }
            spsp_segment_row& s = segs.back();
            s.end = end; ++s.windows; s.keys += keys[w]; s.hit_keys += hit_keys[w]; s.support += call[w] == none ? 0u : support[w];
            m.keys += keys[w]; m.hit_keys += hit_keys[w]; m.called_windows += call[w] != none;
        }
        m.segments = (uint32_t)(segs.size() - seg0);
        order.clear();
        for (size_t s = seg0; s < segs.size(); ++s) if (segs[s].call != none) order.emplace_back(segs[s].call, (uint32_t)(s - seg0));
        std::sort(order.begin(), order.end());
        for (size_t a = 0; a < order.size();) {            // one call's segments: its windows and owned bases
            size_t z = a;
            uint64_t b = 0; uint32_t w = 0;
            for (; z < order.size() && order[z].first == order[a].first; ++z) { const spsp_segment_row& s = segs[seg0 + order[z].second]; b += s.end - s.begin; w += s.windows; }
            const uint32_t c = order[a].first;
            ++m.calls;
            // (calls come in ascending order: only MORE bases displace, so among equals the lower number stays)
            if (m.major == SPSP_WINDOWS_ABSENT || b > m.major_bases) {
                m.second = m.major; m.second_bases = m.major_bases; m.second_windows = m.major_windows;
                m.major = c; m.major_bases = b; m.major_windows = w;
            } else if (m.second == SPSP_WINDOWS_ABSENT || b > m.second_bases) {
                m.second = c; m.second_bases = b; m.second_windows = w;
            }
            a = z;
        }
        mosaic[r] = m;
    }
    spsp_segment_row* o = (spsp_segment_row*)malloc(segs.empty() ? 1 : segs.size() * sizeof(spsp_segment_row));
    if (!o) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    if (!segs.empty()) memcpy(o, segs.data(), segs.size() * sizeof(spsp_segment_row));
    *segments = o; *n_segments = segs.size();
    return SPSP_OK;
}

extern "C" int spsp_segments_csv_host(const spsp_segment_row* segments, uint64_t n_segments, const char* const* record_names, uint32_t n_rec,
                                      const char* const* call_names, const char* last_name, uint32_t n_bins, char** text, uint64_t* len) {
    using namespace spsp;
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!text || !len || !last_name || (n_segments && (!segments || !record_names)) || (n_bins > 1 && !call_names)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_bins == 0) { set_error("windows: n_bins must be 1 or more"); return SPSP_ERR_ARG; }
    std::string s = "record,name,segment,begin,end,windows,call,call_name,keys,hit_keys,support\n";
    for (uint64_t i = 0; i < n_segments; ++i) {
        const spsp_segment_row& g = segments[i];
        if (g.record >= n_rec || g.call >= n_bins) { set_error("windows: segment %llu names record %u or call %u out of range", (unsigned long long)i, g.record, g.call); return SPSP_ERR_ARG; }
        const bool none = g.call + 1 == n_bins;
        s += std::to_string(g.record) + "," + record_names[g.record] + "," + std::to_string(g.segment) + "," + std::to_string(g.begin) + "," + std::to_string(g.end) + "," +
             std::to_string(g.windows) + "," + (none ? std::string(last_name) : std::to_string(g.call)) + "," + (none ? last_name : call_names[g.call]) + "," +
             std::to_string(g.keys) + "," + std::to_string(g.hit_keys) + "," + std::to_string(g.support) + "\n";
    }
    return give_text(s, text, len);
}

extern "C" int spsp_mosaic_csv_host(const spsp_mosaic_row* mosaic, uint32_t n_rec, const char* const* record_names, const char* const* call_names,
                                    const char* last_name, uint32_t n_bins, int precision, char** text, uint64_t* len) {
    using namespace spsp;
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!text || !len || !last_name || (n_rec && (!mosaic || !record_names)) || (n_bins > 1 && !call_names)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_bins == 0) { set_error("windows: n_bins must be 1 or more"); return SPSP_ERR_ARG; }
    std::string s = "record,name,length,windows,segments,called_windows,calls,major,major_name,major_windows,major_bases,f_major,second,second_name,second_windows,"
                    "second_bases,keys,hit_keys\n";
    char buf[64];
    for (uint32_t r = 0; r < n_rec; ++r) {
        const spsp_mosaic_row& m = mosaic[r];
        for (const uint32_t c : {m.major, m.second})
            if (c != SPSP_WINDOWS_ABSENT && c + 1 >= n_bins) { set_error("windows: record %u names call %u, n_bins = %u", r, c, n_bins); return SPSP_ERR_ARG; }
        s += std::to_string(r) + "," + record_names[r] + "," + std::to_string(m.length) + "," + std::to_string(m.windows) + "," + std::to_string(m.segments) + "," +
             std::to_string(m.called_windows) + "," + std::to_string(m.calls) + ",";
        if (m.major != SPSP_WINDOWS_ABSENT) s += std::to_string(m.major) + "," + call_names[m.major] + "," + std::to_string(m.major_windows) + "," + std::to_string(m.major_bases) + ",";
        else s += ",,0,0,";
        s.append(buf, (size_t)format_g(buf, sizeof(buf), precision, m.length ? (double)m.major_bases / (double)m.length : 0.0));
        if (m.second != SPSP_WINDOWS_ABSENT) s += "," + std::to_string(m.second) + "," + call_names[m.second] + "," + std::to_string(m.second_windows) + "," + std::to_string(m.second_bases);
        else s += ",,,0,0";
        s += "," + std::to_string(m.keys) + "," + std::to_string(m.hit_keys) + "\n";
    }
    return give_text(s, text, len);
}

extern "C" int spsp_windows_word_check_host(const char* what, int taxonomy) {
    SplitWord word; uint32_t d = 0;
    const int rc = split_word_for(what, taxonomy != 0, &word, &d);
    if (rc && what) {                                      // (the split's refusals, under this pass's name)
        const std::string said = spsp_last_error();
        if (said.compare(0, 7, "split: ") == 0) spsp::set_error("windows: %s", said.c_str() + 7);
    }
    return rc;
}

// ------------------------------------------------------------------------------------------------- segments as sequence
// The host forms behind the windows (the rule: include/spsp.h, "segments as sequence"): the smoothing of stray runs, the
// selection's word and flags, and the FASTA text as plain loops, which the device writer is held against.

extern "C" int spsp_segments_plan_host(uint32_t* line_bases, uint32_t* stretch_bytes) {
    if (line_bases) *line_bases = spsp::kSgLine;
    if (stretch_bytes) *stretch_bytes = spsp::kSgStretch;
    return SPSP_OK;
}

extern "C" int spsp_windows_smooth_host(uint32_t* call, uint32_t* support, const uint32_t* first_win, uint32_t n_rec, uint32_t n_bins, uint32_t q, uint64_t* n_changed) {
    using namespace spsp;
    if (n_changed) *n_changed = 0;
    if (!first_win || (n_rec && first_win[n_rec] && (!call || !support))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (q > 0x7fffffffu) { set_error("segments: the smoothing must be 0 .. 2147483647 (q = %u)", q); return SPSP_ERR_ARG; }
    for (uint32_t r = 0; r < n_rec; ++r) {                 // (everything is held before anything is changed)
        if (first_win[r] > first_win[r + 1]) { set_error("segments: first_win must not decrease (record %u)", r); return SPSP_ERR_ARG; }
        for (uint32_t w = first_win[r]; w < first_win[r + 1]; ++w)
            if (call[w] >= n_bins) { set_error("segments: record %u, window %u: call %u, n_bins = %u", r, w - first_win[r], call[w], n_bins); return SPSP_ERR_ARG; }
    }
    uint64_t changed = 0;
    std::vector<uint32_t> start;                           // one record's runs: run j = windows [start[j], start[j + 1])
    for (uint32_t r = 0; q && r < n_rec; ++r) {
        const uint32_t w0 = first_win[r], w1 = first_win[r + 1];
        start.clear();
        for (uint32_t w = w0; w < w1; ++w) if (w == w0 || call[w] != call[w - 1]) start.push_back(w);
        start.push_back(w1);
        const size_t n_runs = start.size() - 1;
        // the runs were found on the unsmoothed calls, and a changed run's neighbours are longer than q: they stay as they were
        for (size_t j = 1; j + 1 < n_runs; ++j) {
            const uint32_t len = start[j + 1] - start[j], left = start[j] - start[j - 1], right = start[j + 2] - start[j + 1];
            if (len > q || left <= q || right <= q || call[start[j - 1]] != call[start[j + 1]]) continue;
            for (uint32_t w = start[j]; w < start[j + 1]; ++w) { call[w] = call[start[j - 1]]; support[w] = 0; }
            changed += len;
        }
    }
    if (n_changed) *n_changed = changed;
    return SPSP_OK;
}

namespace {

enum SgWord { kSgAll, kSgCalled, kSgNone, kSgCall, kSgNot, kSgMajor, kSgMinor };

// a decimal of digits alone that stays below `limit`
bool sg_decimal(const char* s, uint64_t limit, uint64_t* v) {
    if (!*s) return false;
    uint64_t x = 0;
    for (; *s; ++s) {
        if (*s < '0' || *s > '9' || x > (limit - (uint64_t)(*s - '0')) / 10) return false;
        x = x * 10 + (uint64_t)(*s - '0');
    }
    if (x >= limit) return false;
    *v = x;
    return true;
}

// what: a word, or <word>:<min_bases> where min is not null.  n_bins == 0: the bins are not counted yet
int sg_word_for(const char* what, bool taxonomy, uint32_t n_bins, SgWord* word, uint32_t* b, uint64_t* min) {
    using namespace spsp;
    if (!what) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    std::string w = what;
    const size_t colon = w.find(':');
    if (colon != std::string::npos) {
        uint64_t m = 0;
        if (!min || !sg_decimal(w.c_str() + colon + 1, 1ull << 63, &m)) {
            set_error("segments: '%s': the least length behind the ':' must be a decimal number below 2^63", what);
            return SPSP_ERR_ARG;
        }
        *min = m;
        w.resize(colon);
    }
    *b = 0;
    if (w == "all") *word = kSgAll;
    else if (w == "called") *word = kSgCalled;
    else if (w == "none") *word = kSgNone;
    else if (w == "major") *word = kSgMajor;
    else if (w == "minor") *word = kSgMinor;
    else if (w.compare(0, 5, "call=") == 0 || w.compare(0, 4, "not=") == 0) {
        const bool is_call = w[0] == 'c';
        uint64_t v = 0;
        if (!sg_decimal(w.c_str() + (is_call ? 5 : 4), 0xffffffffull, &v)) { set_error("segments: '%s': <b> must be a decimal number", what); return SPSP_ERR_ARG; }
        if (n_bins && v + 1 >= n_bins) {
            set_error("segments: '%s': there are %u %s(s), numbered from 0", what, n_bins - 1, taxonomy ? "node" : "reference");
            return SPSP_ERR_ARG;
        }
        *word = is_call ? kSgCall : kSgNot;
        *b = (uint32_t)v;
    } else {
        set_error("segments: '%s' is no word (all, called, none, call=<b>, not=<b>, major, minor)", what);
        return SPSP_ERR_ARG;
    }
    return SPSP_OK;
}

}  // namespace

extern "C" int spsp_segments_word_check_host(const char* what, int taxonomy, uint32_t n_bins) {
    SgWord word; uint32_t b = 0; uint64_t min = 1;
    return sg_word_for(what, taxonomy != 0, n_bins, &word, &b, &min);
}

extern "C" int spsp_segments_select_host(const spsp_segment_row* segments, uint64_t n_segments, const spsp_mosaic_row* mosaic, uint32_t n_rec, uint32_t n_bins,
                                         const char* what, uint64_t min_bases, uint8_t* keep, uint64_t* n_kept, uint64_t* n_bases) {
    using namespace spsp;
    if (n_kept) *n_kept = 0;
    if (n_bases) *n_bases = 0;
    if (!what || (n_segments && (!segments || !keep)) || (n_rec && !mosaic)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_bins == 0) { set_error("segments: n_bins must be 1 or more"); return SPSP_ERR_ARG; }
    if (min_bases >> 63) { set_error("segments: the least length must be below 2^63"); return SPSP_ERR_ARG; }
    SgWord word; uint32_t b = 0;
    if (const int rc = sg_word_for(what, false, n_bins, &word, &b, nullptr)) return rc;
    const uint32_t none = n_bins - 1;
    const uint64_t least = min_bases ? min_bases : 1;
    for (uint64_t i = 0; i < n_segments; ++i) {
        const spsp_segment_row& g = segments[i];
        if (g.record >= n_rec || g.call >= n_bins || g.end < g.begin) {
            set_error("segments: segment %llu names record %u or call %u out of range, or ends in front of its begin", (unsigned long long)i, g.record, g.call);
            return SPSP_ERR_ARG;
        }
    }
    uint64_t kept = 0, bases = 0;
    for (uint64_t i = 0; i < n_segments; ++i) {
        const spsp_segment_row& g = segments[i];
        const uint32_t major = mosaic[g.record].major;
        bool k = false;
        switch (word) {
            case kSgAll: k = true; break;
            case kSgCalled: k = g.call != none; break;
            case kSgNone: k = g.call == none; break;
            case kSgCall: k = g.call == b; break;
            case kSgNot: k = g.call != b; break;
            case kSgMajor: k = major != SPSP_WINDOWS_ABSENT && g.call == major; break;
            case kSgMinor: k = major != SPSP_WINDOWS_ABSENT && g.call != none && g.call != major; break;
        }
        k = k && g.end - g.begin >= least;
        keep[i] = k ? 1 : 0;
        if (k) { ++kept; bases += g.end - g.begin; }
    }
    if (n_kept) *n_kept = kept;
    if (n_bases) *n_bases = bases;
    return SPSP_OK;
}

namespace spsp {
// '>' name ':' begin + 1 '-' end ' ' call_name '\n'
void segment_header(const spsp_segment_row& g, const char* name, const char* const* call_names, const char* last_name, uint32_t n_bins, std::string* s) {
    *s += ">";
    *s += name;
    *s += ":" + std::to_string(g.begin + 1) + "-" + std::to_string(g.end) + " ";
    *s += g.call + 1 == n_bins ? last_name : call_names[g.call];
    *s += "\n";
}
}  // namespace spsp

extern "C" int spsp_segments_fasta_host(const uint8_t* bases, uint64_t n_bases, const uint64_t* rec_off, uint32_t n_rec, const spsp_segment_row* segments,
                                        uint64_t n_segments, const uint8_t* keep, const char* const* record_names, const char* const* call_names,
                                        const char* last_name, uint32_t n_bins, char** text, uint64_t* len) {
    using namespace spsp;
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!text || !len || !last_name || !rec_off || (n_bases && !bases) || (n_segments && (!segments || !record_names)) || (n_bins > 1 && !call_names)) {
        set_error("NULL argument");
        return SPSP_ERR_ARG;
    }
    if (n_bins == 0) { set_error("segments: n_bins must be 1 or more"); return SPSP_ERR_ARG; }
    for (uint32_t r = 0; r < n_rec; ++r)
        if (rec_off[r] > rec_off[r + 1] || rec_off[r + 1] > n_bases) { set_error("segments: the offsets must not decrease and must end inside the bases (record %u)", r); return SPSP_ERR_ARG; }
    std::string s;
    for (uint64_t i = 0; i < n_segments; ++i) {
        const spsp_segment_row& g = segments[i];
        if (g.record >= n_rec || g.call >= n_bins || g.begin > g.end || g.end > rec_off[g.record + 1] - rec_off[g.record]) {
            set_error("segments: segment %llu names record %u or call %u out of range, or leaves its record", (unsigned long long)i, g.record, g.call);
            return SPSP_ERR_ARG;
        }
        if ((keep && !keep[i]) || g.begin == g.end) continue;
        segment_header(g, record_names[g.record], call_names, last_name, n_bins, &s);
        const uint8_t* at = bases + rec_off[g.record] + g.begin;
        const uint64_t n = g.end - g.begin;
        for (uint64_t p = 0; p < n; ++p) {
            const uint8_t c = at[p];
            s += (char)(c >= 'a' && c <= 'z' ? c - 32 : c);
            if ((p + 1) % SPSP_SEGMENTS_LINE == 0 || p + 1 == n) s += '\n';
        }
    }
    return give_text(s, text, len);
}

// ---- raw coordinates (the rule: include/spsp.h, "raw coordinates")

extern "C" int spsp_lift_plan_host(uint32_t* tile_bytes, uint32_t* chunk_bytes) {
    if (tile_bytes) *tile_bytes = spsp::kLfTile;
    if (chunk_bytes) *chunk_bytes = spsp::kLfChunk;
    return SPSP_OK;
}

// the rule as plain loops, a line at a time
extern "C" int spsp_records_lift_host(const uint8_t* text, uint64_t n, const uint64_t* h_base, uint64_t n_q, uint64_t* raw, uint32_t* rec, uint64_t* raw_length,
                                      uint32_t* n_rec) {
    using namespace spsp;
    if (!n_rec || (n && !text) || (n_q && (!h_base || !raw))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    const uint32_t cap = raw_length ? *n_rec : 0u;
    *n_rec = 0;
    for (uint64_t q = 1; q < n_q; ++q)
        if (h_base[q] < h_base[q - 1]) { set_error("lift: the base indices must not decrease (index %llu)", (unsigned long long)q); return SPSP_ERR_ARG; }
    const bool fastq = n > 0 && text[0] == '@';
    std::vector<uint64_t> lens;
    uint64_t kept = 0, seq = 0, q = 0, line = 0, p = 0;
    while (p < n) {
        const uint8_t* nl = (const uint8_t*)memchr(text + p, '\n', (size_t)(n - p));
        const uint64_t e = nl ? (uint64_t)(nl - text) : n;
        bool data;
        if (fastq) {
            // line 4r begins record r, unless it is empty (the blank tail of a text): it is no sequence line either way
            if (line % 4 == 0 && line > 0 && text[p] != '\n' && text[p] != '\r') { lens.push_back(seq); seq = 0; }
            data = line % 4 == 1;
        } else {
            const bool begins = line == 0 || text[p] == '>' || text[p] == 0xFFu;
            if (begins && line > 0) { lens.push_back(seq); seq = 0; }
            data = !begins;
        }
        if (data)
            for (uint64_t i = p; i < e; ++i) {
                const uint8_t c = text[i];
                if (c < 0x21 || c > 0x7e) continue;
                const uint8_t u = c & 0xDFu;
                if (u == 'A' || u == 'C' || u == 'G' || u == 'T') {
                    for (; q < n_q && h_base[q] == kept; ++q) { raw[q] = seq; if (rec) rec[q] = (uint32_t)lens.size(); }
                    ++kept;
                }
                ++seq;
            }
        p = e + 1;
        ++line;
    }
    lens.push_back(seq);
    if (lens.size() > 0xfffffff0ull) { set_error("too many records for one call"); return SPSP_ERR_OVERFLOW; }
    *n_rec = (uint32_t)lens.size();
    if (q < n_q) { set_error("lift: base index %llu is not below the %llu bases", (unsigned long long)h_base[q], (unsigned long long)kept); return SPSP_ERR_ARG; }
    if (raw_length) {
        if (cap != *n_rec) { set_error("lift: the text holds %u record(s), raw_length has room for %u", *n_rec, cap); return SPSP_ERR_ARG; }
        memcpy(raw_length, lens.data(), lens.size() * 8);
    }
    return SPSP_OK;
}

// name, raw_begin, raw_end, call_name, 0, ., segment, begin, end, windows, support -- BED6 and five columns, tab-separated
extern "C" int spsp_segments_bed_host(const spsp_segment_row* segments, uint64_t n_segments, const uint64_t* raw_begin, const uint64_t* raw_end,
                                      const char* const* record_names, uint32_t n_rec, const char* const* call_names, const char* last_name, uint32_t n_bins, char** text,
                                      uint64_t* len) {
    using namespace spsp;
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!text || !len || !last_name || (n_segments && (!segments || !record_names || !raw_begin || !raw_end)) || (n_bins > 1 && !call_names)) {
        set_error("NULL argument");
        return SPSP_ERR_ARG;
    }
    if (n_bins == 0) { set_error("segments: n_bins must be 1 or more"); return SPSP_ERR_ARG; }
    std::string s;
    for (uint64_t i = 0; i < n_segments; ++i) {
        const spsp_segment_row& g = segments[i];
        if (g.record >= n_rec || g.call >= n_bins || g.begin > g.end) {
            set_error("segments: segment %llu names record %u or call %u out of range, or ends in front of its begin", (unsigned long long)i, g.record, g.call);
            return SPSP_ERR_ARG;
        }
        if (g.begin == g.end) continue;                    // no bases: no raw interval
        if (raw_end[i] <= raw_begin[i] || raw_end[i] - raw_begin[i] < g.end - g.begin) {
            set_error("segments: the raw interval of segment %llu is shorter than its %llu base(s)", (unsigned long long)i, (unsigned long long)(g.end - g.begin));
            return SPSP_ERR_ARG;
        }
        std::string call = g.call + 1 == n_bins ? last_name : call_names[g.call];
        for (char& c : call) if (c == '\t') c = ' ';
        s += std::string(record_names[g.record]) + "\t" + std::to_string(raw_begin[i]) + "\t" + std::to_string(raw_end[i]) + "\t" + call + "\t0\t.\t" +
             std::to_string(g.segment) + "\t" + std::to_string(g.begin) + "\t" + std::to_string(g.end) + "\t" + std::to_string(g.windows) + "\t" + std::to_string(g.support) + "\n";
    }
    return give_text(s, text, len);
}
