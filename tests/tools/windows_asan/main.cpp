// The host half of the windows pass -- the counting rule (spsp_records_windows_host), the expansion as plain loops
// (spsp_windows_expand_host), the segments and mosaic rows with their refusals (spsp_windows_segments_host), the two texts
// (spsp_segments_csv_host, spsp_mosaic_csv_host), the word check and the plan -- driven on the CPU by a program of its own, so that
// it can be built with AddressSanitizer + UBSan (run.sh).  No device, no Python.  Every buffer handed in has its exact size on the
// heap: a read behind bases[n - 1], rec_off[n_rec], first_win[n_rec] or call[n_windows - 1] is ASan's to find.
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
};
static bool said(const char* word) { return strstr(spsp_last_error(), word) != nullptr; }

// the rule once more, written from include/spsp.h with nothing shared: the windows of one record as (begin, end) pairs
static std::vector<std::pair<uint64_t, uint64_t>> model(uint64_t L, uint32_t k, uint64_t W) {
    const uint64_t S = W - (k - 1);
    uint64_t n = 1;
    if (L >= k) { n = (L - k + 1 + S - 1) / S; if (n < 1) n = 1; }
    std::vector<std::pair<uint64_t, uint64_t>> w;
    for (uint64_t i = 0; i < n; ++i) w.emplace_back(i * S, i * S + W < L ? i * S + W : L);
    return w;
}

static void expansion(uint32_t k, uint64_t W, const std::vector<uint64_t>& lens, uint64_t seed) {
    std::vector<uint64_t> off{0};
    for (uint64_t L : lens) off.push_back(off.back() + L);
    std::vector<uint8_t> bases((size_t)off.back());
    for (size_t i = 0; i < bases.size(); ++i) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; bases[i] = "ACGT"[seed >> 62]; }
    Exact<uint8_t> b(bases);
    Exact<uint64_t> o(off);
    const uint32_t n_rec = (uint32_t)lens.size();
    Exact<uint32_t> first(std::vector<uint32_t>(n_rec + 1, 7u));
    uint8_t* out = nullptr; uint64_t n_out = 0, n_win = 0; uint64_t* win_off = nullptr;
    CHECK(spsp_windows_expand_host(b.n ? b.p : nullptr, o.p, n_rec, k, W, &out, &n_out, first.p, &win_off, &n_win) == SPSP_OK);
    uint64_t w = 0, at = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        CHECK(first.p[r] == w);
        const auto ws = model(lens[r], k, W);
        std::vector<int> covered((size_t)lens[r], 0);
        for (size_t i = 0; i < ws.size(); ++i, ++w) {
            CHECK(win_off[w] == at);
            if (i + 1 < ws.size()) CHECK(ws[i].second - ws[i].first == W);
            for (uint64_t p = ws[i].first; p < ws[i].second; ++p) CHECK(out[at++] == bases[(size_t)(off[r] + p)]);
            for (uint64_t p = ws[i].first; p + k <= ws[i].second; ++p) ++covered[(size_t)p];
        }
        for (uint64_t p = 0; p + k <= lens[r]; ++p) CHECK(covered[(size_t)p] == 1);   // every k-mer in exactly one window
    }
    CHECK(first.p[n_rec] == w && n_win == w && win_off[w] == at && n_out == at);
    // the counting rule alone gives the same table
    Exact<uint32_t> first2(std::vector<uint32_t>(n_rec + 1, 9u));
    uint64_t* win_off2 = nullptr; uint64_t n_win2 = 0, n_bases2 = 0;
    CHECK(spsp_records_windows_host(o.p, n_rec, k, W, first2.p, &win_off2, &n_win2, &n_bases2) == SPSP_OK && n_win2 == n_win && n_bases2 == n_out);
    CHECK(!memcmp(first.p, first2.p, (n_rec + 1) * 4) && !memcmp(win_off, win_off2, (size_t)(n_win + 1) * 8));
    free(out); free(win_off); free(win_off2);
}

int main() {
    uint32_t a = 0, b = 0, c = 0;
    CHECK(spsp_windows_plan_host(&a, &b, &c) == SPSP_OK && a == spsp::kWnStretch && b == spsp::kWnStretchPacked && c == spsp::kWnRecTile);
    CHECK(spsp_windows_plan_host(nullptr, nullptr, nullptr) == SPSP_OK);
    for (uint32_t k : {5u, 7u, 31u})
        for (uint64_t W : {(uint64_t)k, (uint64_t)k + 1, (uint64_t)k + 9, (uint64_t)200}) {
            const uint64_t S = W - (k - 1);
            expansion(k, W, {0, k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 0, 0, 3 * W + 2, 1}, 17 * k + W);
            expansion(k, W, {}, 1);
            expansion(k, W, {0}, 1);
        }
    // the refusals of the counting rule
    {
        Exact<uint64_t> o(std::vector<uint64_t>{0, 10});
        Exact<uint32_t> first(std::vector<uint32_t>(2, 0));
        uint64_t* win_off = nullptr; uint64_t n_win = 0, n_bases = 0;
        CHECK(spsp_records_windows_host(o.p, 1, 7, 6, first.p, &win_off, &n_win, &n_bases) == SPSP_ERR_ARG && said("width") && !win_off);
        CHECK(spsp_records_windows_host(o.p, 1, 7, 0x80000000ull, first.p, &win_off, &n_win, &n_bases) == SPSP_ERR_ARG && said("width") && !win_off);
        Exact<uint64_t> big(std::vector<uint64_t>{0, 1ull << 40});
        CHECK(spsp_records_windows_host(big.p, 1, 7, 7, first.p, &win_off, &n_win, &n_bases) == SPSP_ERR_OVERFLOW && !win_off);
        Exact<uint64_t> down(std::vector<uint64_t>{5, 3});
        CHECK(spsp_records_windows_host(down.p, 1, 7, 7, first.p, &win_off, &n_win, &n_bases) == SPSP_ERR_ARG && said("decrease"));
    }
    // segments and mosaic: k = 5, W = 8, S = 4; records of 18 (4 windows), 4 (1 window, no keys), 12 (2 windows) bases
    {
        const uint32_t k = 5; const uint64_t W = 8;
        Exact<uint64_t> o(std::vector<uint64_t>{0, 18, 22, 34});
        Exact<uint32_t> first(std::vector<uint32_t>{0, 4, 5, 7});
        Exact<uint32_t> call(std::vector<uint32_t>{0, 1, 1, 2, 2, 2, 1}), keys(std::vector<uint32_t>{3, 4, 5, 6, 0, 2, 2}), hit(std::vector<uint32_t>{1, 2, 3, 0, 0, 0, 1}),
            sup(std::vector<uint32_t>{1, 2, 2, 9, 9, 9, 1});
        Exact<spsp_mosaic_row> mos(std::vector<spsp_mosaic_row>(3));
        spsp_segment_row* seg = nullptr; uint64_t n_seg = 0;
        CHECK(spsp_windows_segments_host(call.p, keys.p, hit.p, sup.p, first.p, o.p, 3, k, W, 3, &seg, &n_seg, mos.p) == SPSP_OK && n_seg == 6);
        // record 0: [0,4) call 0, [4,12) call 1, [12,18) none; record 1: [0,4) none; record 2: [0,4) none, [4,12) call 1
        CHECK(seg[0].begin == 0 && seg[0].end == 4 && seg[0].call == 0 && seg[0].support == 1 && seg[1].begin == 4 && seg[1].end == 12 && seg[1].windows == 2 &&
              seg[1].keys == 9 && seg[1].hit_keys == 5 && seg[1].support == 4 && seg[2].begin == 12 && seg[2].end == 18 && seg[2].call == 2 && seg[2].support == 0);
        CHECK(seg[3].record == 1 && seg[3].segment == 0 && seg[3].end == 4 && seg[4].record == 2 && seg[4].call == 2 && seg[5].segment == 1 && seg[5].end == 12);
        CHECK(mos.p[0].calls == 2 && mos.p[0].major == 1 && mos.p[0].major_bases == 8 && mos.p[0].second == 0 && mos.p[0].second_bases == 4 && mos.p[0].called_windows == 3 &&
              mos.p[0].segments == 3 && mos.p[0].keys == 18 && mos.p[1].calls == 0 && mos.p[1].major == SPSP_WINDOWS_ABSENT && mos.p[2].major == 1 &&
              mos.p[2].second == SPSP_WINDOWS_ABSENT);
        const char* rn[3] = {"a", "b", "c"};
        const char* cn[2] = {"X", "Y"};
        char* text = nullptr; uint64_t len = 0;
        CHECK(spsp_segments_csv_host(seg, n_seg, rn, 3, cn, "unmatched", 3, &text, &len) == SPSP_OK && len == strlen(text) && strstr(text, "\n0,a,1,4,12,2,1,Y,9,5,4\n"));
        free(text);
        CHECK(spsp_mosaic_csv_host(mos.p, 3, rn, cn, "unmatched", 3, 6, &text, &len) == SPSP_OK && len == strlen(text) &&
              strstr(text, "\n0,a,18,4,3,3,2,1,Y,2,8,0.444444,0,X,1,4,18,6\n") && strstr(text, "\n1,b,4,1,1,0,0,,,0,0,0,,,0,0,0,0\n"));
        free(text);
        seg[1].call = 3;
        CHECK(spsp_segments_csv_host(seg, n_seg, rn, 3, cn, "unmatched", 3, &text, &len) == SPSP_ERR_ARG && !text);
        free(seg);
        // the refusals: a call >= n_bins, first_win against the rule -- each names its record
        call.p[5] = 3;
        CHECK(spsp_windows_segments_host(call.p, keys.p, hit.p, sup.p, first.p, o.p, 3, k, W, 3, &seg, &n_seg, mos.p) == SPSP_ERR_ARG && said("record 2") && !seg);
        call.p[5] = 2; first.p[2] = 6;
        CHECK(spsp_windows_segments_host(call.p, keys.p, hit.p, sup.p, first.p, o.p, 3, k, W, 3, &seg, &n_seg, mos.p) == SPSP_ERR_ARG && said("record 1") && !seg);
        first.p[2] = 5;
        CHECK(spsp_windows_segments_host(call.p, keys.p, hit.p, sup.p, first.p, o.p, 3, k, 4, 3, &seg, &n_seg, mos.p) == SPSP_ERR_ARG && said("width"));
        // no record at all
        Exact<uint64_t> o0(std::vector<uint64_t>{0});
        Exact<uint32_t> f0(std::vector<uint32_t>{0});
        CHECK(spsp_windows_segments_host(nullptr, nullptr, nullptr, nullptr, f0.p, o0.p, 0, k, W, 3, &seg, &n_seg, nullptr) == SPSP_OK && n_seg == 0);
        free(seg);
    }
    CHECK(spsp_windows_word_check_host("best", 0) == SPSP_OK && spsp_windows_word_check_host("taxon", 1) == SPSP_OK && spsp_windows_word_check_host("depth=3", 1) == SPSP_OK);
    CHECK(spsp_windows_word_check_host("best", 1) == SPSP_ERR_ARG && said("windows") && spsp_windows_word_check_host("depth=0", 1) == SPSP_ERR_ARG &&
          spsp_windows_word_check_host("nearest", 0) == SPSP_ERR_ARG && said("nearest") && spsp_windows_word_check_host(nullptr, 0) == SPSP_ERR_ARG);
    printf("windows_asan: ok\n");
    return 0;
}
