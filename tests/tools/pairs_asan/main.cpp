// The host half of the paired records -- the naming rule (spsp_pairs_names_host) and the union's plan (spsp_union_plan_host) --
// driven on the CPU by a program of its own, so that it can be built with AddressSanitizer + UBSan (run.sh).  No device, no
// Python.  Every name handed in sits in a heap block of exactly its size (and its 0 byte): a read in front of names[p][0] or
// behind the 0 byte is ASan's to find -- the rule looks at the last two bytes of names of every length.
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

// names in heap blocks of exactly their sizes
struct Names {
    std::vector<char*> p;
    explicit Names(const std::vector<std::string>& names) {
        for (const std::string& s : names) {
            char* c = (char*)malloc(s.size() + 1);
            memcpy(c, s.c_str(), s.size() + 1);
            p.push_back(c);
        }
    }
    ~Names() { for (char* c : p) free(c); }
    const char* const* data() const { return p.data(); }
};

// the rule over two lists: the call's return code, *bad, and the common names where it gives them
static int rule(const std::vector<std::string>& n1, const std::vector<std::string>& n2, uint64_t* bad, std::vector<std::string>* common) {
    CHECK(n1.size() == n2.size());
    Names a(n1), b(n2);
    char* blob = nullptr;
    const int rc = spsp_pairs_names_host(n1.empty() ? nullptr : a.data(), n2.empty() ? nullptr : b.data(), n1.size(), common ? &blob : nullptr, bad);
    if (common) {
        common->clear();
        if (rc == SPSP_OK) {
            CHECK(blob != nullptr);
            size_t at = 0;
            for (size_t p = 0; p < n1.size(); ++p) { common->emplace_back(blob + at); at += common->back().size() + 1; }
            spsp_free(blob);
        } else CHECK(blob == nullptr);
    }
    return rc;
}

int main() {
    using S = std::vector<std::string>;
    uint32_t threads = 0, tile = 0;
    CHECK(spsp_union_plan_host(&threads, &tile) == SPSP_OK && threads == spsp::kUnThreads && tile == spsp::kUnTile);
    CHECK(spsp_union_plan_host(nullptr, nullptr) == SPSP_OK && spsp_union_plan_host(&threads, nullptr) == SPSP_OK);

    uint64_t bad = 99;
    S common;
    CHECK(rule({}, {}, &bad, &common) == SPSP_OK && bad == 0 && common.empty());
    CHECK(rule({"r1/1", "r2/1"}, {"r1/2", "r2/2"}, &bad, &common) == SPSP_OK && bad == 2 && common == S({"r1", "r2"}));
    CHECK(rule({"r1", "x.7"}, {"r1", "x.7"}, &bad, &common) == SPSP_OK && common == S({"r1", "x.7"}));
    CHECK(rule({"r1/1", "r2"}, {"r1", "r2/2"}, &bad, &common) == SPSP_OK && common == S({"r1", "r2"}));
    CHECK(rule({"a/1/1"}, {"a/1/2"}, &bad, &common) == SPSP_OK && common == S({"a/1"}));
    // names of 0, 1 and 2 bytes: the suffix test looks two bytes back
    CHECK(rule({"", "1", "/", "/1", "/1"}, {"", "1", "/", "/2", ""}, &bad, &common) == SPSP_OK && common == S({"", "1", "/", "", ""}));
    CHECK(rule({"r1/1"}, {"r1/1"}, &bad, &common) == SPSP_ERR_FORMAT && bad == 0 && common.empty());
    CHECK(strstr(spsp_last_error(), "pair 0") && strstr(spsp_last_error(), "'r1/1'"));
    CHECK(rule({"r1/2"}, {"r1/2"}, &bad, nullptr) == SPSP_ERR_FORMAT && bad == 0);
    CHECK(rule({"a", "b", "c/1", "d", "e"}, {"a", "b", "d/2", "e", "f"}, &bad, &common) == SPSP_ERR_FORMAT && bad == 2);
    CHECK(strstr(spsp_last_error(), "pair 2") && strstr(spsp_last_error(), "'c/1'") && strstr(spsp_last_error(), "'d/2'"));
    CHECK(rule({"a", "b"}, {"a", "B"}, &bad, nullptr) == SPSP_ERR_FORMAT && bad == 1);
    CHECK(rule({"ab"}, {"a"}, &bad, nullptr) == SPSP_ERR_FORMAT && rule({"a"}, {"ab"}, &bad, nullptr) == SPSP_ERR_FORMAT);
    CHECK(rule({"1"}, {"2"}, &bad, nullptr) == SPSP_ERR_FORMAT && rule({"/"}, {""}, &bad, nullptr) == SPSP_ERR_FORMAT);
    // a name longer than the error text has room for
    const std::string longer(5000, 'x');
    CHECK(rule({longer + "/1"}, {longer + "/2"}, &bad, &common) == SPSP_OK && common == S({longer}));
    CHECK(rule({longer + "a"}, {longer + "b"}, &bad, &common) == SPSP_ERR_FORMAT && bad == 0 && strlen(spsp_last_error()) < 1024);
    // every cut of a name against itself and against its suffixed forms
    const std::string whole = "read.12/1";
    for (size_t cut = 0; cut <= whole.size(); ++cut) {
        const std::string part = whole.substr(0, cut);
        const int rc = rule({part}, {part}, &bad, &common);
        const bool ends_1 = cut >= 2 && part.compare(cut - 2, 2, "/1") == 0;
        CHECK(rc == (ends_1 ? SPSP_ERR_FORMAT : SPSP_OK));
        CHECK(rule({part + "/1"}, {part + "/2"}, &bad, &common) == SPSP_OK && common == S({part}));
    }
    // the refusals of the call itself
    Names one(S({"a"}));
    CHECK(spsp_pairs_names_host(one.data(), one.data(), 1, nullptr, nullptr) == SPSP_ERR_ARG);
    CHECK(spsp_pairs_names_host(nullptr, one.data(), 1, nullptr, &bad) == SPSP_ERR_ARG && spsp_pairs_names_host(one.data(), nullptr, 1, nullptr, &bad) == SPSP_ERR_ARG);
    const char* hole[1] = {nullptr};
    CHECK(spsp_pairs_names_host(hole, one.data(), 1, nullptr, &bad) == SPSP_ERR_ARG);
    CHECK(spsp_pairs_names_host(nullptr, nullptr, 0, nullptr, &bad) == SPSP_OK && bad == 0);
    printf("pairs_asan: ok\n");
    return 0;
}
