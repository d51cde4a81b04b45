// The host half of the selection -- the sketch writer (spsp_sketch_from_keys_host), the band parser (spsp_select_band_host) and
// the reader's round trip (spsp_sketch_parse_host, spsp_sketch_header_host) -- driven on the CPU by a program of its own, so that
// it can be built with AddressSanitizer + UBSan (run.sh).  No device, no Python.  Keys are hand-built: a minimizer planted at the
// first, a middle and the last place of random k-mers, a minimizer that is its own reverse complement, a k-mer that holds the
// minimizer on both strands, two keys of one minimizer beside a lone one, and no keys at all.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
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

static u128 revcomp(u128 v, uint32_t n) {                  // A=0 C=1 T=2 G=3: complement = code ^ 2
    u128 r = 0;
    for (uint32_t i = 0; i < n; ++i) { r = (r << 2) | ((v & 3) ^ 2); v >>= 2; }
    return r;
}

typedef std::tuple<uint32_t, uint64_t, uint64_t> Key;      // (minimizer, kmer_hi, kmer_lo): the order of the arrays

static Key plant(u128 kmer, uint32_t mn, uint32_t at, uint32_t k, uint32_t m) {
    const u128 kmask = (((u128)1) << (2 * k)) - 1, mmask = (((u128)1) << (2 * m)) - 1;
    const uint32_t sh = 2 * (k - m - at);
    kmer = ((kmer & kmask) & ~(mmask << sh)) | ((u128)mn << sh);
    const u128 rc = revcomp(kmer, k), c = kmer < rc ? kmer : rc;
    return Key(mn, (uint64_t)(c >> 64), (uint64_t)c);
}

static void round_trip(std::vector<Key> keys, uint32_t k, uint32_t m, double rate) {
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::vector<uint32_t> mn;
    std::vector<uint64_t> lo, hi;
    for (auto& x : keys) { mn.push_back(std::get<0>(x)); hi.push_back(std::get<1>(x)); lo.push_back(std::get<2>(x)); }
    uint8_t* payload = nullptr; uint64_t len = 0;
    CHECK(spsp_sketch_from_keys_host(k, m, rate, mn.data(), lo.data(), k > 32 ? hi.data() : nullptr, keys.size(), &payload, &len) == SPSP_OK);
    uint32_t kk = 0, mm = 0; uint64_t cnt = 0, n = 0; double r = 0;
    CHECK(spsp_sketch_header_host(payload, len, &kk, &mm, &cnt, &r) == SPSP_OK && kk == k && mm == m && cnt == keys.size() && r == rate);
    uint32_t* a = nullptr; uint64_t *b = nullptr, *c = nullptr;
    CHECK(spsp_sketch_parse_host(payload, len, &kk, &mm, &a, &b, &c, &n) == SPSP_OK && kk == k && mm == m && n == keys.size());
    for (uint64_t i = 0; i < n; ++i) CHECK(a[i] == mn[i] && b[i] == lo[i] && c[i] == hi[i]);
    spsp::ParsedSketch P;
    CHECK(spsp::sketch_parse_structure_host(payload, len, &P) == SPSP_OK && P.n_keys == keys.size() && P.k == k && P.m == m);
    free(a); free(b); free(c); free(payload);
}

int main() {
    std::mt19937_64 rng(20);
    const uint32_t shapes[][2] = {{31, 11}, {63, 15}, {32, 15}, {33, 15}, {21, 9}, {12, 11}, {2, 1}};
    for (auto& km : shapes) {
        const uint32_t k = km[0], m = km[1];
        const uint32_t mmask = (uint32_t)((1ull << (2 * m)) - 1);
        std::vector<Key> keys;
        for (int t = 0; t < 600; ++t) {
            const u128 kmer = ((u128)rng() << 64) | rng();
            const uint32_t at = t % 3 == 0 ? 0 : t % 3 == 1 ? (k - m) / 2 : k - m;
            keys.push_back(plant(kmer, (uint32_t)rng() & mmask, at, k, m));
        }
        // a minimizer that is its own reverse complement (ATAT..: A <-> T), m even only
        if (m % 2 == 0) { uint32_t p = 0; for (uint32_t j = 0; j < m; ++j) p = (p << 2) | (j % 2 ? 2u : 0u); keys.push_back(plant(rng(), p, 1 % (k - m + 1), k, m)); }
        // a k-mer that holds the minimizer on both strands: the minimizer at the front, its reverse complement at the back
        if (k >= 2 * m) {
            const uint32_t mn = (uint32_t)rng() & mmask;
            u128 kmer = ((u128)rng() << 64) | rng();
            kmer = (kmer & ~(u128)mmask) | revcomp(mn, m);
            keys.push_back(plant(kmer, mn, 0, k, m));
        }
        // two keys of one minimizer and a lone one
        keys.push_back(plant(1, 5 & mmask, 0, k, m)); keys.push_back(plant(~(u128)0, 5 & mmask, k - m, k, m)); keys.push_back(plant(77, 2 & mmask, 0, k, m));
        round_trip(keys, k, m, 100.0);
        round_trip(std::vector<Key>(keys.begin(), keys.begin() + 1), k, m, 1.0);
        round_trip({}, k, m, 1000.0);
        // the refusals: out of order, a key twice, a minimizer that is not in the k-mer, k == m
        uint8_t* payload = nullptr; uint64_t len = 0;
        const uint32_t two_mn[2] = {3 & mmask, 1 & mmask};
        const uint64_t two[2] = {std::get<2>(plant(0, 3 & mmask, 0, k, m)), std::get<2>(plant(0, 1 & mmask, 0, k, m))}, zero[2] = {0, 0};
        if (k <= 32) CHECK(spsp_sketch_from_keys_host(k, m, 100.0, two_mn, two, nullptr, 2, &payload, &len) == SPSP_ERR_ARG && !payload);
        const uint32_t same_mn[2] = {0, 0};
        CHECK(spsp_sketch_from_keys_host(k, m, 100.0, same_mn, zero, zero, 2, &payload, &len) == SPSP_ERR_ARG && !payload);
        const uint32_t g = mmask;                                     // GGG...: not in AAA... nor in TTT...
        CHECK(spsp_sketch_from_keys_host(k, m, 100.0, &g, zero, zero, 1, &payload, &len) == SPSP_ERR_ARG && strstr(spsp_last_error(), "key 0"));
        CHECK(spsp_sketch_from_keys_host(m, m, 100.0, same_mn, zero, zero, 1, &payload, &len) == SPSP_ERR_ARG && strstr(spsp_last_error(), "k == m"));
    }
    // the band parser
    struct { const char* what; uint32_t R, a, b; } bands[] = {
        {"union", 20, 1, 20}, {"present", 1, 1, 1}, {"absent", 7, 0, 0}, {"all", 1, 1, 1}, {"all", 65535, 65535, 65535},
        {"core=0.05", 20, 1, 20}, {"unique=0.05", 20, 1, 0}, {"shell=0.05", 20, 1, 0}, {"core=0.9", 20, 18, 20}, {"shell=0.9", 20, 2, 17},
        {"unique=0.9", 20, 1, 1}, {"shell=0.1", 20, 1, 0}, {"core=1", 65535, 65535, 65535}, {"core=0.999999", 65535, 65535, 65535},
        {"core=0.000001", 65535, 1, 65535}, {"3..7", 9, 3, 7}, {"7..3", 9, 7, 3}, {"0..4294967295", 2, 0, 0xffffffffu}};
    for (auto& c : bands) {
        uint32_t a = 9, b = 9;
        CHECK(spsp_select_band_host(c.what, c.R, &a, &b) == SPSP_OK && a == c.a && b == c.b);
    }
    const char* garbage[] = {"", "core", "core=", "core=0", "core=1.5", "core=0.1234567", "core=.5", "kernel=0.5", "union=0.5", "1..", "..2", "1...2", "1..2..3",
                             "4294967296..5", "-1..2", "5", " union", "Union", "core=0.5 ", "1 ..2", "99999999999..1"};
    for (const char* w : garbage) {
        uint32_t a = 9, b = 9;
        CHECK(spsp_select_band_host(w, 5, &a, &b) == SPSP_ERR_ARG && a == 1 && b == 0);
    }
    uint32_t a = 0, b = 0;
    CHECK(spsp_select_band_host("union", 0, &a, &b) == SPSP_ERR_ARG && spsp_select_band_host(nullptr, 3, &a, &b) == SPSP_ERR_ARG);
    printf("select_asan ok\n");
    return 0;
}
