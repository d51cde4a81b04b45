// The host half of "segments as sequence" -- the smoothing (spsp_windows_smooth_host), the selection (spsp_segments_select_host,
// spsp_segments_word_check_host), the FASTA text as plain loops (spsp_segments_fasta_host) and the plan -- driven on the CPU by a
// program of its own, so that it can be built with AddressSanitizer + UBSan (run.sh).  No device, no Python.  Every buffer handed
// in has its exact size on the heap: a read behind call[n_windows - 1], first_win[n_rec], keep[n_segments - 1] or bases[n - 1] is
// ASan's to find.
#include <algorithm>
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../supersampler_amd/csrc/spsp_internal.h"

// what spsp_host.cpp takes from the device side of the library: never reached from here
namespace spsp {
static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
int compare_payloads_impl(spsp_ctx*, const uint8_t* const*, const uint64_t*, uint32_t, const int*, const uint32_t*, uint32_t, const uint64_t*, uint32_t*, uint32_t*, uint32_t*, uint64_t*, bool*, std::vector<uint64_t>*) { return SPSP_ERR_NO_DEVICE; }
int compare_payloads_multi(spsp_ctx* const*, uint32_t, const uint8_t* const*, const uint64_t*, uint32_t, const int*, const uint32_t*, uint32_t, const uint64_t*, uint32_t*, uint32_t*, uint32_t*, uint64_t*, bool*, std::vector<uint64_t>*) { return SPSP_ERR_NO_DEVICE; }
int check_params(const spsp_params*) { return SPSP_ERR_NO_DEVICE; }
}  // namespace spsp
extern "C" {
const char* spsp_last_error(void) { return spsp::g_err.c_str(); }
void spsp_free(void* p) { free(p); }
int spsp_create(int, void*, spsp_ctx**) { return SPSP_ERR_NO_DEVICE; }
void spsp_destroy(spsp_ctx*) {}
}

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, spsp_last_error()); exit(1); } \
    } while (0)

// a copy of `v` in a heap block of exactly its size
template <class T> struct Exact {
    T* p;
    size_t n;
    explicit Exact(const std::vector<T>& v) : p((T*)malloc(v.size() ? v.size() * sizeof(T) : 1)), n(v.size()) { if (n) memcpy(p, v.data(), n * sizeof(T)); }
    ~Exact() { free(p); }
    std::vector<T> vec() const { return std::vector<T>(p, p + n); }
};
static bool said(const char* word) { return strstr(spsp_last_error(), word) != nullptr; }

// the rule once more, written from include/spsp.h with nothing shared: the runs of one record, the stray ones changed
static void model_smooth(std::vector<uint32_t>& call, std::vector<uint32_t>& support, const std::vector<uint32_t>& first, uint32_t q, uint64_t* changed) {
    const std::vector<uint32_t> old = call;
    *changed = 0;
    for (size_t r = 0; q && r + 1 < first.size(); ++r) {
        std::vector<std::pair<uint32_t, uint32_t>> runs;   // (start, length)
        for (uint32_t w = first[r]; w < first[r + 1]; ++w) {
            if (runs.empty() || old[w] != old[w - 1]) runs.emplace_back(w, 0u);
            ++runs.back().second;
        }
        for (size_t j = 1; j + 1 < runs.size(); ++j)
            if (runs[j].second <= q && runs[j - 1].second > q && runs[j + 1].second > q && old[runs[j - 1].first] == old[runs[j + 1].first])
                for (uint32_t w = runs[j].first; w < runs[j].first + runs[j].second; ++w) { call[w] = old[runs[j - 1].first]; support[w] = 0; ++*changed; }
    }
}

static void smooth_case(const std::vector<uint32_t>& call, const std::vector<uint32_t>& first, uint32_t n_bins, uint32_t q) {
    std::vector<uint32_t> support(call.size());
    for (size_t w = 0; w < call.size(); ++w) support[w] = 100 + (uint32_t)w;
    std::vector<uint32_t> want_c = call, want_s = support;
    uint64_t want_n = 0, got_n = 77;
    model_smooth(want_c, want_s, first, q, &want_n);
    Exact<uint32_t> c(call), s(support), f(first);
    CHECK(spsp_windows_smooth_host(c.p, s.p, f.p, (uint32_t)first.size() - 1, n_bins, q, &got_n) == SPSP_OK);
    CHECK(c.vec() == want_c && s.vec() == want_s && got_n == want_n);
}

static spsp_segment_row seg(uint32_t record, uint32_t segment, uint64_t begin, uint64_t end, uint32_t call) {
    spsp_segment_row g{};
    g.record = record; g.segment = segment; g.begin = begin; g.end = end; g.call = call; g.windows = 1;
    return g;
}

int main() {
    uint32_t line = 0, stretch = 0;
    CHECK(spsp_segments_plan_host(&line, &stretch) == SPSP_OK && line == SPSP_SEGMENTS_LINE && stretch == 16384);
    CHECK(spsp_segments_plan_host(nullptr, nullptr) == SPSP_OK);

    // smoothing: hand-made vectors at the rule's seams, then seeded ones
    const uint32_t none = 3;
    smooth_case({0, 0, 0, 1, 0, 0, 0}, {0, 7}, 4, 0);
    smooth_case({0, 0, 0, 1, 0, 0, 0}, {0, 7}, 4, 1);
    smooth_case({0, 0, 1, 1, 0, 0}, {0, 6}, 4, 1);
    smooth_case({0, 0, 1, 1, 0, 0}, {0, 6}, 4, 2);         // the flanks have exactly q windows: nothing changes
    smooth_case({0, 0, 0, 1, 1, 0, 0, 0}, {0, 8}, 4, 2);
    smooth_case({1, 0, 0, 0, 2}, {0, 5}, 4, 1);            // strays at the record's ends
    smooth_case({0, 0, 1, 2, 2}, {0, 5}, 4, 1);            // neighbours that differ
    smooth_case({0, 0, none, 0, 0, none, none, 1, none, none}, {0, 10}, 4, 1);
    smooth_case({0, 0, 1, 0, 0, 0, 0}, {0, 3, 7}, 4, 1);   // a run that ends with its record borrows no flank from the next
    smooth_case({0, 1, 2, 0}, {0, 1, 2, 3, 4}, 4, 3);      // records of one window
    smooth_case({}, {0}, 4, 5);
    smooth_case({}, {0, 0, 0}, 4, 5);
    smooth_case({0, 0, 0, 1, 0, 0, 0}, {0, 7}, 4, 0x7fffffffu);
    uint64_t x = 88172645463325252ull;
    const auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int round = 0; round < 40; ++round) {
        std::vector<uint32_t> first(1, 0), call;
        const uint32_t n_rec = 1 + (uint32_t)(rnd() % 8), stay = 2 + (uint32_t)(rnd() % 6);
        for (uint32_t r = 0; r < n_rec; ++r) {
            const uint32_t n = (uint32_t)(rnd() % 60);
            uint32_t c = (uint32_t)(rnd() % 4);
            for (uint32_t w = 0; w < n; ++w) { if (rnd() % stay == 0) c = (uint32_t)(rnd() % 4); call.push_back(c); }
            first.push_back((uint32_t)call.size());
        }
        smooth_case(call, first, 4, (uint32_t)(rnd() % 4));
    }
    {
        const std::vector<uint32_t> call{0, 0, 4, 0}, first{0, 2, 4}, down{0, 3, 2};
        Exact<uint32_t> c(call), s(call), f(first), d(down);
        uint64_t n = 5;
        CHECK(spsp_windows_smooth_host(c.p, s.p, f.p, 2, 4, 1, &n) == SPSP_ERR_ARG && said("record 1") && n == 0 && c.vec() == call);
        CHECK(spsp_windows_smooth_host(c.p, s.p, d.p, 2, 5, 1, &n) == SPSP_ERR_ARG && said("record 1"));
        CHECK(spsp_windows_smooth_host(c.p, s.p, f.p, 2, 5, 0x80000000u, &n) == SPSP_ERR_ARG);
        CHECK(spsp_windows_smooth_host(c.p, s.p, nullptr, 2, 5, 1, &n) == SPSP_ERR_ARG);
        CHECK(spsp_windows_smooth_host(c.p, s.p, f.p, 2, 5, 1, nullptr) == SPSP_OK);
    }

    // the words
    for (const char* w : {"all", "called", "none", "call=0", "not=2", "major", "minor", "all:0", "call=1:100", "minor:9223372036854775807"})
        CHECK(spsp_segments_word_check_host(w, 0, 4) == SPSP_OK);
    CHECK(spsp_segments_word_check_host("call=4000000000", 1, 0) == SPSP_OK);
    for (const char* w : {"", "bogus", "ALL", "call=", "call=x", "call=-1", "call=3", "not=3", "not=1x", "call=4294967295", "all:", "all:x", "all:1:2",
                          "all:9223372036854775808", "all:-1", "major=1", " all"})
        CHECK(spsp_segments_word_check_host(w, 0, 4) == SPSP_ERR_ARG && said("segments"));
    CHECK(spsp_segments_word_check_host(nullptr, 0, 4) == SPSP_ERR_ARG);

    // the selection: record 0 with major 1, record 1 without a major, record 2 empty
    std::vector<spsp_segment_row> segs{seg(0, 0, 0, 10, 1), seg(0, 1, 10, 14, none), seg(0, 2, 14, 20, 0), seg(0, 3, 20, 50, 1), seg(1, 0, 0, 7, none), seg(2, 0, 0, 0, none)};
    std::vector<spsp_mosaic_row> mos(3);
    mos[0].major = 1; mos[0].second = 0; mos[1].major = mos[1].second = mos[2].major = mos[2].second = SPSP_WINDOWS_ABSENT;
    const auto select = [&](const char* what, uint64_t min, const std::vector<uint8_t>& want, uint64_t want_bases) {
        Exact<spsp_segment_row> g(segs);
        Exact<spsp_mosaic_row> m(mos);
        Exact<uint8_t> keep(std::vector<uint8_t>(segs.size(), 9));
        uint64_t n = 0, b = 0, w = 0;
        CHECK(spsp_segments_select_host(g.p, g.n, m.p, 3, 4, what, min, keep.p, &n, &b) == SPSP_OK);
        for (uint8_t k : want) w += k;
        CHECK(keep.vec() == want && n == w && b == want_bases);
    };
    select("all", 1, {1, 1, 1, 1, 1, 0}, 57);
    select("all", 0, {1, 1, 1, 1, 1, 0}, 57);
    select("called", 1, {1, 0, 1, 1, 0, 0}, 46);
    select("none", 1, {0, 1, 0, 0, 1, 0}, 11);
    select("call=1", 1, {1, 0, 0, 1, 0, 0}, 40);
    select("not=1", 1, {0, 1, 1, 0, 1, 0}, 17);
    select("major", 1, {1, 0, 0, 1, 0, 0}, 40);
    select("minor", 1, {0, 0, 1, 0, 0, 0}, 6);
    select("all", 9, {1, 0, 0, 1, 0, 0}, 40);
    select("all", 10, {1, 0, 0, 1, 0, 0}, 40);
    select("all", 11, {0, 0, 0, 1, 0, 0}, 30);
    {
        Exact<spsp_segment_row> g(segs);
        Exact<spsp_mosaic_row> m(mos);
        Exact<uint8_t> keep(std::vector<uint8_t>(segs.size(), 9));
        uint64_t n = 0, b = 0;
        CHECK(spsp_segments_select_host(g.p, g.n, m.p, 3, 4, "call=3", 1, keep.p, &n, &b) == SPSP_ERR_ARG);
        CHECK(spsp_segments_select_host(g.p, g.n, m.p, 3, 4, "all:5", 1, keep.p, &n, &b) == SPSP_ERR_ARG);
        CHECK(spsp_segments_select_host(g.p, g.n, m.p, 3, 4, "all", 1ull << 63, keep.p, &n, &b) == SPSP_ERR_ARG);
        CHECK(spsp_segments_select_host(g.p, g.n, m.p, 2, 4, "all", 1, keep.p, &n, &b) == SPSP_ERR_ARG);   // record 2 of two
        CHECK(spsp_segments_select_host(g.p, g.n, m.p, 3, 3, "all", 1, keep.p, &n, &b) == SPSP_ERR_ARG);   // call 3 of three bins
        CHECK(spsp_segments_select_host(nullptr, 0, nullptr, 0, 1, "all", 1, nullptr, &n, &b) == SPSP_OK && n == 0);
    }

    // the text: bodies of the lengths around a line, lower case folded, the last bin's name
    {
        const std::vector<uint64_t> lens{1, 79, 80, 81, 159, 160, 161, 0};
        std::vector<uint64_t> off(1, 0);
        std::vector<uint8_t> bases;
        for (uint64_t L : lens) { for (uint64_t i = 0; i < L; ++i) bases.push_back((uint8_t)"ACGTacgt"[rnd() % 8]); off.push_back(bases.size()); }
        std::vector<spsp_segment_row> all;
        std::vector<std::string> names;
        for (uint32_t r = 0; r < lens.size(); ++r) { all.push_back(seg(r, 0, 0, lens[r], r % 3)); names.push_back("rec " + std::to_string(r)); }
        all.push_back(seg(6, 1, 80, 161, 2));
        std::vector<const char*> np;
        for (const std::string& s : names) np.push_back(s.c_str());
        const char* calls[2] = {"ref A", "refB"};
        std::string want;
        for (const spsp_segment_row& g : all) {
            if (g.begin == g.end) continue;
            want += ">" + names[g.record] + ":" + std::to_string(g.begin + 1) + "-" + std::to_string(g.end) + " " + (g.call == 2 ? "unmatched" : calls[g.call]) + "\n";
            for (uint64_t p = g.begin; p < g.end; ++p) {
                want += (char)toupper(bases[off[g.record] + p]);
                if ((p - g.begin) % 80 == 79 || p + 1 == g.end) want += '\n';
            }
        }
        Exact<uint8_t> b(bases);
        Exact<uint64_t> o(off);
        Exact<spsp_segment_row> g(all);
        char* text = nullptr; uint64_t len = 0;
        CHECK(spsp_segments_fasta_host(b.p, b.n, o.p, (uint32_t)lens.size(), g.p, g.n, nullptr, np.data(), calls, "unmatched", 3, &text, &len) == SPSP_OK);
        CHECK(std::string(text, len) == want);
        uint64_t body = 0;
        for (uint64_t L : lens) body += L + (L + 79) / 80;
        CHECK(std::count(want.begin(), want.end(), '>') == 8 && body + 81 + 2 < len);
        spsp_free(text);
        Exact<uint8_t> keep(std::vector<uint8_t>{0, 0, 1, 0, 0, 0, 0, 1, 0});
        CHECK(spsp_segments_fasta_host(b.p, b.n, o.p, (uint32_t)lens.size(), g.p, g.n, keep.p, np.data(), calls, "unmatched", 3, &text, &len) == SPSP_OK);
        CHECK(len == strlen(">rec 2:1-80 unmatched\n") + 81 && text[len - 1] == '\n');
        spsp_free(text);
        std::vector<spsp_segment_row> bad{seg(0, 0, 0, 2, 0)};   // leaves its record of one base
        Exact<spsp_segment_row> gb(bad);
        CHECK(spsp_segments_fasta_host(b.p, b.n, o.p, (uint32_t)lens.size(), gb.p, 1, nullptr, np.data(), calls, "unmatched", 3, &text, &len) == SPSP_ERR_ARG && !text);
        CHECK(spsp_segments_fasta_host(b.p, b.n - 1, o.p, (uint32_t)lens.size(), g.p, g.n, nullptr, np.data(), calls, "unmatched", 3, &text, &len) == SPSP_ERR_ARG);
        CHECK(spsp_segments_fasta_host(nullptr, 0, o.p, 0, nullptr, 0, nullptr, nullptr, nullptr, "unmatched", 1, &text, &len) == SPSP_OK && len == 0);
        spsp_free(text);
    }
    printf("segments_asan: ok\n");
    return 0;
}
