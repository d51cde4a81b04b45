// The host half of the linkage tree -- the ordering step behind the device pass (spsp::tree_rows_host), spsp_tree_cut_host,
// spsp_tree_csv_host, spsp_tree_newick_host -- driven on the CPU by a program of its own, so that it can be built with
// AddressSanitizer + UBSan (run.sh).  No device, no Python.  It checks what is cheap to check on the way: the rows' order by
// 128-bit cross products, the sizes, the cut's counts, the texts' ends, and that bad rows are refused.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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
        if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } \
    } while (0)

static uint64_t under(int metric, const std::vector<uint64_t>& card, uint32_t a, uint32_t b, uint64_t x) {
    return metric == SPSP_CLUSTER_JACCARD ? card[a] + card[b] - x : (card[a] < card[b] ? card[a] : card[b]);
}

// a random spanning forest over n sketches (every sketch after the first hangs on an earlier one, or starts a component), shuffled
static void one_forest(std::mt19937_64& rng, uint32_t n, uint64_t card_max, int metric, int precision) {
    std::vector<uint64_t> card(n);
    for (auto& c : card) c = card_max / 2 + rng() % (card_max / 2);
    std::vector<uint64_t> forest;
    for (uint32_t b = 1; b < n; ++b) {
        if (rng() % 7 == 0) continue;
        const uint32_t a = (uint32_t)(rng() % b);
        const uint64_t lim = std::min<uint64_t>(std::min(card[a], card[b]), 0xffffffffull);
        const uint64_t x = rng() % 3 == 0 ? lim / 2 + 1 : 1 + rng() % lim;   // (a third of the edges share one count: equal fractions)
        forest.push_back((uint64_t)a << 48 | (uint64_t)b << 32 | x);
    }
    for (size_t i = forest.size(); i > 1; --i) std::swap(forest[i - 1], forest[rng() % i]);
    std::vector<spsp_tree_row> rows(n ? n - 1 : 0);
    CHECK(spsp::tree_rows_host(forest.data(), forest.size(), card.data(), n, metric, rows.data()) == SPSP_OK);
    for (size_t r = 0; r + 1 < forest.size(); ++r) {
        const spsp_tree_row &p = rows[r], &q = rows[r + 1];
        const u128 l = (u128)p.shared * under(metric, card, q.a, q.b, q.shared), m = (u128)q.shared * under(metric, card, p.a, p.b, p.shared);
        CHECK(l > m || (l == m && ((uint64_t)p.a << 16 | p.b) < ((uint64_t)q.a << 16 | q.b)));
        CHECK(p.a < p.b && p.b < n && p.size >= 2 && p.size <= n && p.reserved == 0);
    }
    std::vector<std::string> name_text(n);
    std::vector<const char*> names(n);
    for (uint32_t i = 0; i < n; ++i) { name_text[i] = (i % 5 == 0 ? "it's " : "s") + std::to_string(i) + (i % 3 == 0 ? ":(,)" : ""); names[i] = name_text[i].c_str(); }
    std::vector<uint32_t> cluster(n);
    uint64_t count = 0, floor_count = 0;
    CHECK(spsp_tree_cut_host(rows.data(), forest.size(), n, card.data(), metric, 0, 1, 0, 1, cluster.data(), &floor_count) == SPSP_OK);
    CHECK(floor_count == n - forest.size() && cluster[0] == 0);
    for (uint32_t num : {1u, 250000u, 500000u, 999999u, 1000000u}) {
        CHECK(spsp_tree_cut_host(rows.data(), forest.size(), n, card.data(), metric, 0, 1000000, num, 1000000, cluster.data(), &count) == SPSP_OK);
        CHECK(count >= floor_count && count <= n);
        floor_count = count;                               // (a higher cut never has fewer clusters)
    }
    char* text = nullptr; uint64_t len = 0;
    CHECK(spsp_tree_csv_host(rows.data(), forest.size(), names.data(), n, card.data(), metric, precision, &text, &len) == SPSP_OK);
    CHECK(len > 10 && text[len - 1] == '\n');
    spsp_free(text);
    CHECK(spsp_tree_newick_host(rows.data(), forest.size(), names.data(), n, card.data(), metric, precision, &text, &len) == SPSP_OK);
    CHECK(len >= 3 && text[len - 2] == ';' && text[len - 1] == '\n');
    uint64_t open = 0, close = 0, quotes = 0;
    for (uint64_t i = 0; i < len; ++i) { quotes += text[i] == '\''; if (quotes % 2 == 0) { open += text[i] == '('; close += text[i] == ')'; } }
    CHECK(open == close && open == n - 1 && quotes % 2 == 0);
    spsp_free(text);
}

int main() {
    std::mt19937_64 rng(7);
    for (int t = 0; t < 300; ++t) one_forest(rng, 1 + (uint32_t)(rng() % 200), 1000, t & 1, 6);
    for (int t = 0; t < 20; ++t) one_forest(rng, 2 + (uint32_t)(rng() % 50), (1ull << 47) - 1, t & 1, 3);   // products beyond 64 bits
    one_forest(rng, 65535, 100000, SPSP_CLUSTER_JACCARD, 6);
    // the deepest tree there is: a caterpillar over 65 535 sketches
    {
        const uint32_t n = 65535;
        std::vector<uint64_t> card(n, 100000), forest;
        for (uint32_t i = 0; i + 1 < n; ++i) forest.push_back((uint64_t)i << 48 | (uint64_t)(i + 1) << 32 | (uint64_t)(70000 - i));
        std::vector<spsp_tree_row> rows(n - 1);
        CHECK(spsp::tree_rows_host(forest.data(), forest.size(), card.data(), n, SPSP_CLUSTER_CONTAINMENT, rows.data()) == SPSP_OK);
        CHECK(rows[0].a == 0 && rows[n - 2].b == n - 1 && rows[n - 2].size == n);
        std::vector<std::string> name_text(n);
        std::vector<const char*> names(n);
        for (uint32_t i = 0; i < n; ++i) { name_text[i] = "s" + std::to_string(i); names[i] = name_text[i].c_str(); }
        char* text = nullptr; uint64_t len = 0;
        CHECK(spsp_tree_newick_host(rows.data(), n - 1, names.data(), n, card.data(), SPSP_CLUSTER_CONTAINMENT, 6, &text, &len) == SPSP_OK);
        CHECK(len > n && text[0] == '(' && text[n - 2] == '(' && text[n - 1] == '\'');
        spsp_free(text);
    }
    // n = 1, and what is refused
    {
        const uint64_t card[3] = {100, 100, 100};
        const char* names[3] = {"a", "b'", "c"};
        char* text = nullptr; uint64_t len = 0, count = 0;
        uint32_t cluster[3];
        CHECK(spsp_tree_newick_host(nullptr, 0, names, 1, card, 0, 6, &text, &len) == SPSP_OK && len == 5 && !memcmp(text, "'a';\n", 5));
        spsp_free(text);
        CHECK(spsp_tree_newick_host(nullptr, 0, names, 3, card, 0, 6, &text, &len) == SPSP_OK && std::string(text, len) == "(('a':1,'b''':1):0,'c':1);\n");
        spsp_free(text);
        const spsp_tree_row bad[][2] = {{{1, 1, 2, 0, 5}, {0, 2, 3, 0, 5}}, {{0, 3, 2, 0, 5}, {0, 2, 3, 0, 5}}, {{2, 1, 2, 0, 5}, {0, 2, 3, 0, 5}}};
        for (const auto& rows : bad) {
            CHECK(spsp_tree_cut_host(rows, 2, 3, card, 0, 0, 1, 0, 1, cluster, &count) == SPSP_ERR_ARG);
            CHECK(spsp_tree_csv_host(rows, 2, names, 3, card, 0, 6, &text, &len) == SPSP_ERR_ARG);
            CHECK(spsp_tree_newick_host(rows, 2, names, 3, card, 0, 6, &text, &len) == SPSP_ERR_ARG);
        }
        const spsp_tree_row twice[2] = {{0, 1, 2, 0, 5}, {0, 1, 2, 0, 5}};
        CHECK(spsp_tree_newick_host(twice, 2, names, 3, card, 0, 6, &text, &len) == SPSP_ERR_ARG);
        CHECK(spsp_tree_cut_host(twice, 1, 3, card, 0, 1, 2, 1, 3, cluster, &count) == SPSP_ERR_ARG);   // below the floor
        const uint64_t cyc[3] = {0ull << 48 | 1ull << 32 | 5, 1ull << 48 | 2ull << 32 | 5, 0ull << 48 | 2ull << 32 | 5};
        spsp_tree_row out[3];
        CHECK(spsp::tree_rows_host(cyc, 3, card, 3, 0, out) == SPSP_ERR_ARG);
        const uint64_t outside[1] = {0ull << 48 | 3ull << 32 | 5};
        CHECK(spsp::tree_rows_host(outside, 1, card, 3, 0, out) == SPSP_ERR_ARG);
    }
    printf("tree host functions: ok\n");
    return 0;
}
