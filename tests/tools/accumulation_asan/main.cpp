// The host half of the accumulation -- the order generator (spsp_accumulation_orders_host), the pass's plan
// (spsp_accumulation_plan_host) and the CSV writer with its refusals (spsp_accumulation_csv_host) -- driven on the CPU by a program
// of its own, so that it can be built with AddressSanitizer + UBSan (run.sh).  No device, no Python.  The generator is held against
// a second statement of its rule written here: the smallest sizes, one order, and a seed whose first draw is the largest 64-bit
// word, which every bound that is no power of two draws again.
#include <algorithm>
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

typedef unsigned __int128 u128;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, spsp_last_error()); exit(1); } \
    } while (0)

// the rule of include/spsp.h once more, with 128-bit arithmetic where the library wraps 64 bits; *redrawn counts the draws thrown away
static std::vector<uint32_t> orders_again(uint32_t n, uint32_t n_orders, uint64_t seed, uint64_t* redrawn) {
    std::vector<uint32_t> out((size_t)n_orders * n);
    uint64_t s = seed;
    *redrawn = 0;
    for (uint32_t p = 0; p < n_orders; ++p) {
        uint32_t* a = out.data() + (size_t)p * n;
        for (uint32_t i = 0; i < n; ++i) a[i] = i;
        if (p == 0) continue;
        for (uint32_t i = n - 1; i >= 1; --i) {
            const u128 b = (u128)i + 1, two64 = (u128)1 << 64, limit = two64 - two64 % b;
            uint64_t z;
            for (;;) {
                s += 0x9E3779B97F4A7C15ull;
                z = s;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                z ^= z >> 31;
                if ((u128)z < limit) break;
                ++*redrawn;
            }
            std::swap(a[i], a[(uint32_t)((u128)z % b)]);
        }
    }
    return out;
}

static void orders_case(uint32_t n, uint32_t n_orders, uint64_t seed, bool want_redraw) {
    // the exact size on the heap: a write behind the last order is ASan's to find
    uint32_t* got = (uint32_t*)malloc((size_t)n_orders * n * 4);
    CHECK(got && spsp_accumulation_orders_host(n, n_orders, seed, got) == SPSP_OK);
    uint64_t redrawn = 0;
    const std::vector<uint32_t> want = orders_again(n, n_orders, seed, &redrawn);
    CHECK(!memcmp(got, want.data(), want.size() * 4));
    CHECK(!want_redraw || redrawn > 0);
    for (uint32_t p = 0; p < n_orders; ++p) {
        std::vector<uint32_t> sorted(got + (size_t)p * n, got + (size_t)(p + 1) * n);
        std::sort(sorted.begin(), sorted.end());
        for (uint32_t i = 0; i < n; ++i) CHECK(sorted[i] == i && (p != 0 || got[i] == i));
    }
    free(got);
}

static std::string csv(const std::vector<spsp_accumulation_row>& rows, uint32_t n_orders, int precision, int* rc) {
    char* text = nullptr; size_t len = 0;
    *rc = spsp_accumulation_csv_host(rows.data(), (uint32_t)rows.size(), n_orders, precision, &text, &len);
    std::string out = *rc == SPSP_OK ? std::string(text, len) : std::string();
    if (*rc == SPSP_OK) spsp_free(text);
    return out;
}

int main() {
    const uint64_t kRedrawSeed = 3558559446808474027ull;   // its first draw is 2^64 - 1
    orders_case(1, 1, 1, false);
    orders_case(1, 5, 7, false);
    orders_case(2, 1, 1, false);
    orders_case(2, 9, 2, false);
    orders_case(3, 2, kRedrawSeed, true);                  // below(3): 2^64 mod 3 = 1, the largest word is drawn again
    orders_case(1000, 3, kRedrawSeed, true);
    orders_case(1000, 33, 1, false);
    orders_case(65535, 2, 5, false);
    uint32_t word = 0;
    CHECK(spsp_accumulation_orders_host(0, 1, 1, &word) == SPSP_ERR_ARG && spsp_accumulation_orders_host(65536, 1, 1, &word) == SPSP_ERR_ARG);
    CHECK(spsp_accumulation_orders_host(1, 0, 1, &word) == SPSP_ERR_ARG && spsp_accumulation_orders_host(1, 1025, 1, &word) == SPSP_ERR_ARG);
    CHECK(spsp_accumulation_orders_host(1, 1, 1, nullptr) == SPSP_ERR_ARG);
    // the plan: whatever it says fits the LDS it was made for
    for (uint32_t n = 1; n <= 65535; ++n) {
        uint32_t g = 0, w = 0, bits = 0, cut = 0;
        CHECK(spsp_accumulation_plan_host(n, &g, &w, &bits, &cut) == SPSP_OK);
        const uint64_t lds = (uint64_t)g * ((n + 1u) & ~1u) * 2 + (uint64_t)g * w * 4 + (uint64_t)(spsp::kAcPassThreads / 64) * (bits / 8);
        CHECK(g >= 1 && g <= 8 && (g & (g - 1)) == 0 && w >= 1 && w <= n && lds <= spsp::kAcLdsBytes && cut <= 64 && (g == 1 || w == n));
    }
    CHECK(spsp_accumulation_plan_host(0, nullptr, nullptr, nullptr, nullptr) == SPSP_ERR_ARG && spsp_accumulation_plan_host(1, nullptr, nullptr, nullptr, nullptr) == SPSP_OK);
    // the writer: three genomes over two orders
    int rc = 0;
    const std::vector<spsp_accumulation_row> good = {{10, 12, 22, 10, 12, 22, 10, 10}, {15, 15, 30, 4, 7, 11, 15, 7}, {16, 16, 32, 3, 3, 6, 16, 3}};
    const std::string text = csv(good, 2, 6, &rc);
    CHECK(rc == SPSP_OK);
    CHECK(text == "genomes,pan_min,pan_mean,pan_max,core_min,core_mean,core_max,new_mean,pan_listed,core_listed\n"
                  "1,10,11,12,10,11,12,11,10,10\n2,15,15,15,4,5.5,7,4,15,7\n3,16,16,16,3,3,3,1,16,3\n");
    for (int precision : {1, 17}) { csv(good, 2, precision, &rc); CHECK(rc == SPSP_OK); }
    const auto refused = [&](size_t row, void (*spoil)(spsp_accumulation_row&)) {
        std::vector<spsp_accumulation_row> bad = good;
        spoil(bad[row]);
        int r = 0;
        csv(bad, 2, 6, &r);
        return r == SPSP_ERR_ARG;
    };
    CHECK(refused(0, [](spsp_accumulation_row& r) { r.pan_min = 13; }));               // min > max
    CHECK(refused(1, [](spsp_accumulation_row& r) { r.core_min = 8; }));
    CHECK(refused(0, [](spsp_accumulation_row& r) { r.pan_sum = 25; }));               // sum > P * max
    CHECK(refused(0, [](spsp_accumulation_row& r) { r.pan_sum = 19; }));               // sum < P * min
    CHECK(refused(1, [](spsp_accumulation_row& r) { r.core_sum = 15; }));
    CHECK(refused(1, [](spsp_accumulation_row& r) { r.pan_min = 9; r.pan_sum = 24; r.pan_first = 9; }));     // pan_min falls
    CHECK(refused(2, [](spsp_accumulation_row& r) { r.core_max = 8; r.core_sum = 11; }));                    // core_max rises
    CHECK(refused(0, [](spsp_accumulation_row& r) { r.pan_first = 13; }));             // the listed order outside [min, max]
    CHECK(refused(1, [](spsp_accumulation_row& r) { r.core_first = 3; }));
    CHECK(refused(0, [](spsp_accumulation_row& r) { r.pan_max = ~0ull; r.pan_sum = ~0ull; }) == false);      // (P * max beyond 64 bits is weighed in 128)
    char* t = nullptr; size_t l = 0;
    CHECK(spsp_accumulation_csv_host(good.data(), 3, 0, 6, &t, &l) == SPSP_ERR_ARG && spsp_accumulation_csv_host(good.data(), 3, 1025, 6, &t, &l) == SPSP_ERR_ARG);
    CHECK(spsp_accumulation_csv_host(good.data(), 0, 2, 6, &t, &l) == SPSP_ERR_ARG && spsp_accumulation_csv_host(nullptr, 3, 2, 6, &t, &l) == SPSP_ERR_ARG);
    CHECK(spsp_accumulation_csv_host(good.data(), 3, 2, 6, nullptr, &l) == SPSP_ERR_ARG && spsp_accumulation_csv_host(good.data(), 3, 2, 6, &t, nullptr) == SPSP_ERR_ARG);
    printf("accumulation host functions OK\n");
    return 0;
}
