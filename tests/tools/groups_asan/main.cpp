// The host half of the groups pass -- the labels reader (spsp_groups_labels_host), the bounds (spsp_groups_bounds_host) and the two
// CSV writers with their refusals (spsp_groups_csv_host, spsp_groups_members_csv_host) -- driven on the CPU by a program of its
// own, so that it can be built with AddressSanitizer + UBSan (run.sh).  No device, no Python.  Every buffer handed in has its exact
// size on the heap: a read behind a labels text without a final newline, or a write behind group[n - 1], is ASan's to find.
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

// the labels reader on a text of exactly its length: -> rc, the labels and the names as one string with '|' between them
static int labels(const std::string& text, uint32_t n, std::vector<uint32_t>* group, std::string* names) {
    char* exact = (char*)malloc(text.size() ? text.size() : 1);
    memcpy(exact, text.data(), text.size());
    uint32_t* g = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
    uint32_t G = 0;
    char* blob = nullptr; uint64_t blob_len = 0;
    const int rc = spsp_groups_labels_host(text.empty() ? nullptr : exact, text.size(), n, g, &G, &blob, &blob_len);
    group->clear(); names->clear();
    if (rc == SPSP_OK) {
        group->assign(g, g + n);
        uint32_t seen = 0;
        for (uint64_t i = 0; i < blob_len; ++i) { if (blob[i]) *names += blob[i]; else { *names += '|'; ++seen; } }
        CHECK(seen == G);
        spsp_free(blob);
    } else CHECK(blob == nullptr && blob_len == 0 && G == 0);
    free(exact); free(g);
    return rc;
}

static bool refused_at(const std::string& text, uint32_t n, const char* where) {
    std::vector<uint32_t> g; std::string names;
    return labels(text, n, &g, &names) == SPSP_ERR_ARG && strstr(spsp_last_error(), where) != nullptr;
}

static std::string groups_csv(const std::vector<spsp_group_row>& rows, const std::vector<const char*>& names, int precision, int* rc) {
    char* text = nullptr; uint64_t len = 0;
    *rc = spsp_groups_csv_host(rows.data(), (uint32_t)rows.size(), names.data(), precision, &text, &len);
    std::string out = *rc == SPSP_OK ? std::string(text, len) : std::string();
    if (*rc == SPSP_OK) spsp_free(text);
    return out;
}

int main() {
    std::vector<uint32_t> g; std::string names;
    CHECK(labels("b\na\nb\nc c\na\n", 5, &g, &names) == SPSP_OK && g == std::vector<uint32_t>({0, 1, 0, 2, 1}) && names == "b|a|c c|");
    CHECK(labels("b\r\na\r\nb", 3, &g, &names) == SPSP_OK && g == std::vector<uint32_t>({0, 1, 0}) && names == "b|a|");   // \r\n, no final newline
    CHECK(labels("x", 1, &g, &names) == SPSP_OK && names == "x|");
    {
        std::string many;
        for (uint32_t i = 0; i < 65535; ++i) many += "label " + std::to_string(i % 1000) + (i + 1 < 65535 ? "\n" : "");
        CHECK(labels(many, 65535, &g, &names) == SPSP_OK && g[64999] == 999 && g[65534] == 534);
    }
    CHECK(refused_at("a\nb\n", 3, "line 3") && refused_at("a\nb\nc", 2, "line 3") && refused_at("", 1, "line 1") && refused_at("a\n\nb\n", 3, "line 2"));
    CHECK(refused_at("\r\n", 1, "line 1") && refused_at("a\nb,c\n", 2, "line 2") && refused_at("a\n\"\n", 2, "line 2") && refused_at("a\tb", 1, "line 1"));
    CHECK(refused_at(std::string("a\nb\0c\n", 6), 2, "line 2") && refused_at("a\nb\r\r\n", 2, "line 2") && refused_at("a\nb\n\n", 2, "line 3"));
    uint32_t word = 0, G = 0;
    CHECK(spsp_groups_labels_host("a", 1, 0, &word, &G, nullptr, nullptr) == SPSP_ERR_ARG && spsp_groups_labels_host("a", 1, 65536, &word, &G, nullptr, nullptr) == SPSP_ERR_ARG);
    CHECK(spsp_groups_labels_host("a", 1, 1, nullptr, &G, nullptr, nullptr) == SPSP_ERR_ARG && spsp_groups_labels_host("a", 1, 1, &word, nullptr, nullptr, nullptr) == SPSP_ERR_ARG);
    CHECK(spsp_groups_labels_host("a", 1, 1, &word, &G, nullptr, nullptr) == SPSP_OK && G == 1 && word == 0);   // (the names are optional)

    // the bounds at their equalities, in arrays of exactly n_groups words
    const auto bounds = [](const std::vector<uint32_t>& group, uint32_t n_groups, uint32_t num, uint32_t den, uint32_t onum, uint32_t oden,
                           std::vector<uint32_t>* out) {
        uint32_t* a = (uint32_t*)malloc((n_groups ? n_groups : 1) * 4 * 3);
        const int rc = spsp_groups_bounds_host(group.data(), (uint32_t)group.size(), n_groups, num, den, onum, oden, a, a + n_groups, a + 2 * n_groups);
        out->assign(a, a + (rc == SPSP_OK ? 3 * n_groups : 0));
        free(a);
        return rc;
    };
    std::vector<uint32_t> labels50(50, 1), out;
    for (uint32_t i = 0; i < 20; ++i) labels50[i] = 0;
    CHECK(bounds(labels50, 2, 19, 20, 1, 10, &out) == SPSP_OK && out == std::vector<uint32_t>({20, 30, 19, 29, 3, 2}));
    CHECK(bounds({0, 0, 0, 1}, 2, 2, 3, 0, 1, &out) == SPSP_OK && out == std::vector<uint32_t>({3, 1, 2, 1, 0, 0}));
    CHECK(bounds({0, 0, 0, 0, 0, 0, 0}, 1, 1, 1000000, 1, 1, &out) == SPSP_OK && out == std::vector<uint32_t>({7, 1, 0}));
    {
        std::vector<uint32_t> big(65535, 0);
        big[65534] = 1;
        CHECK(bounds(big, 2, 999999, 1000000, 999999, 1000000, &out) == SPSP_OK && out == std::vector<uint32_t>({65534, 1, 65534, 1, 0, 65533}));
    }
    CHECK(bounds({}, 1, 1, 1, 0, 1, &out) == SPSP_ERR_ARG && bounds({0}, 0, 1, 1, 0, 1, &out) == SPSP_ERR_ARG && bounds({0}, 2, 1, 1, 0, 1, &out) == SPSP_ERR_ARG);
    CHECK(bounds({0, 2}, 2, 1, 1, 0, 1, &out) == SPSP_ERR_ARG && bounds({0, 0, 2}, 3, 1, 1, 0, 1, &out) == SPSP_ERR_ARG && strstr(spsp_last_error(), "group 1"));
    CHECK(bounds({0}, 1, 0, 1, 0, 1, &out) == SPSP_ERR_ARG && bounds({0}, 1, 2, 1, 0, 1, &out) == SPSP_ERR_ARG && bounds({0}, 1, 1, 1000001, 0, 1, &out) == SPSP_ERR_ARG);
    CHECK(bounds({0}, 1, 1, 1, 2, 1, &out) == SPSP_ERR_ARG && bounds({0}, 1, 1, 1, 0, 0, &out) == SPSP_ERR_ARG && bounds({0}, 1, 1, 1, 0, 1000001, &out) == SPSP_ERR_ARG);
    CHECK(spsp_groups_bounds_host(labels50.data(), 50, 2, 1, 1, 0, 1, nullptr, nullptr, nullptr) == SPSP_OK);   // (validation only)

    // the writers: the hand-checked example of include/spsp.h and a group of empty sketches behind it
    int rc = 0;
    const std::vector<spsp_group_row> rows = {{3, 11, 5, 4, 2, 1}, {2, 5, 3, 2, 1, 1}, {1, 3, 3, 3, 1, 1}, {2, 0, 0, 0, 0, 0}};
    const std::vector<const char*> gnames = {"ST 131", "clade-B", "x", "empty ones"};
    const std::string text = groups_csv(rows, gnames, 6, &rc);
    CHECK(rc == SPSP_OK);
    CHECK(text == "group,members,keys,present,core,exclusive,marker,f_core,f_marker\nST 131,3,11,5,4,2,1,0.8,0.25\nclade-B,2,5,3,2,1,1,0.666667,0.5\n"
                  "x,1,3,3,3,1,1,1,0.333333\nempty ones,2,0,0,0,0,0,0,0\n");
    for (int precision : {1, 17}) { groups_csv(rows, gnames, precision, &rc); CHECK(rc == SPSP_OK); }
    const auto g_refused = [&](size_t row, void (*spoil)(spsp_group_row&)) {
        std::vector<spsp_group_row> bad = rows;
        spoil(bad[row]);
        int r = 0;
        groups_csv(bad, gnames, 6, &r);
        return r == SPSP_ERR_ARG;
    };
    CHECK(g_refused(0, [](spsp_group_row& r) { r.core = 6; }) && g_refused(1, [](spsp_group_row& r) { r.marker = 3; }));
    CHECK(g_refused(2, [](spsp_group_row& r) { r.exclusive = 4; }) && g_refused(3, [](spsp_group_row& r) { r.core = 1; }));
    char* t = nullptr; uint64_t l = 0;
    CHECK(spsp_groups_csv_host(rows.data(), 0, gnames.data(), 6, &t, &l) == SPSP_ERR_ARG && spsp_groups_csv_host(nullptr, 4, gnames.data(), 6, &t, &l) == SPSP_ERR_ARG);
    CHECK(spsp_groups_csv_host(rows.data(), 4, nullptr, 6, &t, &l) == SPSP_ERR_ARG && spsp_groups_csv_host(rows.data(), 4, gnames.data(), 6, nullptr, &l) == SPSP_ERR_ARG);

    const std::vector<spsp_group_member_row> members = {{3, 2, 1}, {2, 1, 1}, {4, 1, 1}, {2, 1, 1}, {3, 1, 1}, {3, 1, 1}, {0, 0, 0}, {0, 0, 0}};
    const std::vector<uint32_t> group = {0, 1, 0, 1, 0, 2, 3, 3};
    const std::vector<uint64_t> card = {4, 2, 4, 3, 3, 3, 0, 0};
    const std::vector<const char*> snames = {"s0", "s1", "s2", "s3", "s4", "s5", "s6", "s7"};
    const auto members_csv = [&](const std::vector<spsp_group_member_row>& m, const std::vector<uint32_t>& gr, const std::vector<uint64_t>& c, std::string* out) {
        char* text2 = nullptr; uint64_t len = 0;
        const int r = spsp_groups_members_csv_host(m.data(), (uint32_t)m.size(), snames.data(), gr.data(), c.data(), rows.data(), 4, gnames.data(), 6, &text2, &len);
        if (r == SPSP_OK) { out->assign(text2, len); spsp_free(text2); }
        return r;
    };
    std::string mtext;
    CHECK(members_csv(members, group, card, &mtext) == SPSP_OK);
    CHECK(mtext == "sketch,group,keys,core,exclusive,marker,f_core,f_marker\ns0,ST 131,4,3,2,1,0.75,1\ns1,clade-B,2,2,1,1,1,1\ns2,ST 131,4,4,1,1,1,1\n"
                   "s3,clade-B,3,2,1,1,0.666667,1\ns4,ST 131,3,3,1,1,1,1\ns5,x,3,3,1,1,1,1\ns6,empty ones,0,0,0,0,0,0\ns7,empty ones,0,0,0,0,0,0\n");
    const auto m_refused = [&](size_t row, void (*spoil)(spsp_group_member_row&)) {
        std::vector<spsp_group_member_row> bad = members;
        spoil(bad[row]);
        std::string unused;
        return members_csv(bad, group, card, &unused) == SPSP_ERR_ARG;
    };
    CHECK(m_refused(1, [](spsp_group_member_row& r) { r.core = 3; }) && m_refused(3, [](spsp_group_member_row& r) { r.core = 3; }));
    CHECK(m_refused(0, [](spsp_group_member_row& r) { r.exclusive = 3; }) && m_refused(0, [](spsp_group_member_row& r) { r.marker = 2; }));
    CHECK(m_refused(5, [](spsp_group_member_row& r) { r.core = 0; }) && m_refused(6, [](spsp_group_member_row& r) { r.exclusive = 1; }));
    std::string unused;
    CHECK(members_csv(members, {0, 1, 0, 1, 0, 2, 3, 4}, card, &unused) == SPSP_ERR_ARG);
    CHECK(members_csv(members, group, {4, 2, 3, 3, 3, 3, 0, 0}, &unused) == SPSP_ERR_ARG);
    printf("groups host functions OK\n");
    return 0;
}
