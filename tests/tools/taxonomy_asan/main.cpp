// The host half of the taxonomy -- the lineage parser (spsp_taxonomy_lineages_host), the tree check (spsp_taxonomy_check_host), the
// plan (spsp_taxonomy_plan_host) and the two CSV writers with their refusals (spsp_taxonomy_csv_host,
// spsp_taxonomy_report_csv_host) -- driven on the CPU by a program of its own, so that it can be built with AddressSanitizer +
// UBSan (run.sh).  No device, no Python.  Every buffer handed in has its exact size on the heap: a read behind parent[T - 1],
// ref_node[n_ref - 1] or the last name is ASan's to find.
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

// a parsed lineage file in arrays of exactly their sizes
struct Parsed {
    int rc = 0;
    uint32_t T = 0;
    std::vector<uint32_t> parent, depth, size, ref_node;
    std::vector<std::string> names;
};

static Parsed parse(const std::string& text, uint32_t n_ref) {
    Parsed P;
    char* copy = (char*)malloc(text.size() ? text.size() : 1);   // (no 0 byte behind the text)
    memcpy(copy, text.data(), text.size());
    uint32_t* ref = (uint32_t*)malloc((n_ref ? n_ref : 1) * 4);
    uint32_t *parent = nullptr, *depth = nullptr, *size = nullptr;
    char* names = nullptr; uint64_t names_len = 0;
    P.rc = spsp_taxonomy_lineages_host(copy, text.size(), n_ref, ref, &parent, &depth, &size, &names, &names_len, &P.T);
    if (P.rc == SPSP_OK) {
        P.parent.assign(parent, parent + P.T); P.depth.assign(depth, depth + P.T); P.size.assign(size, size + P.T); P.ref_node.assign(ref, ref + n_ref);
        for (uint64_t at = 0; at < names_len; at += strlen(names + at) + 1) P.names.emplace_back(names + at);
        CHECK(P.names.size() == P.T);
    } else CHECK(!parent && !depth && !size && !names && P.T == 0);
    spsp_free(parent); spsp_free(depth); spsp_free(size); spsp_free(names);
    free(copy); free(ref);
    return P;
}

static int check(const std::vector<uint32_t>& parent, const std::vector<uint32_t>& ref_node) {
    uint32_t* p = (uint32_t*)malloc((parent.size() ? parent.size() : 1) * 4);
    uint32_t* r = (uint32_t*)malloc((ref_node.size() ? ref_node.size() : 1) * 4);
    if (!parent.empty()) memcpy(p, parent.data(), parent.size() * 4);
    if (!ref_node.empty()) memcpy(r, ref_node.data(), ref_node.size() * 4);
    const int rc = spsp_taxonomy_check_host(p, (uint32_t)parent.size(), r, (uint32_t)ref_node.size());
    free(p); free(r);
    return rc;
}

struct Row { uint64_t length; uint32_t keys, hit_keys, node, start, score, clade, direct, winners; };

// both writers on arrays of exactly their sizes: -> rc of the first (the second must agree), the two texts
static int write_both(const std::vector<Row>& rows, const Parsed& P, int precision, std::string* csv, std::string* report) {
    const size_t n = rows.size();
    spsp_taxonomy_record* rec = (spsp_taxonomy_record*)malloc((n ? n : 1) * sizeof(spsp_taxonomy_record));
    std::vector<std::string> rn(n);
    const char** rp = (const char**)malloc((n ? n : 1) * sizeof(char*));
    const char** np = (const char**)malloc((P.T ? P.T : 1) * sizeof(char*));
    uint32_t* parent = (uint32_t*)malloc((P.T ? P.T : 1) * 4);
    uint32_t* ref = (uint32_t*)malloc((P.ref_node.size() ? P.ref_node.size() : 1) * 4);
    memcpy(parent, P.parent.data(), (size_t)P.T * 4);
    memcpy(ref, P.ref_node.data(), P.ref_node.size() * 4);
    for (size_t r = 0; r < n; ++r) {
        const Row& w = rows[r];
        rec[r].length = w.length; rec[r].keys = w.keys; rec[r].hit_keys = w.hit_keys; rec[r].node = w.node; rec[r].start = w.start; rec[r].score = w.score;
        rec[r].clade = w.clade; rec[r].direct = w.direct; rec[r].winners = w.winners;
        rn[r] = "rec" + std::to_string(r); rp[r] = rn[r].c_str();
    }
    for (uint32_t t = 0; t < P.T; ++t) np[t] = P.names[t].c_str();
    char* text = nullptr; uint64_t len = 0;
    const int rc = spsp_taxonomy_csv_host(n ? rec : nullptr, n, rp, parent, P.T, np, precision, &text, &len);
    csv->clear(); report->clear();
    if (rc == SPSP_OK) { csv->assign(text, len); spsp_free(text); }
    text = nullptr; len = 0;
    const int rc2 = spsp_taxonomy_report_csv_host(n ? rec : nullptr, n, parent, P.T, np, ref, (uint32_t)P.ref_node.size(), &text, &len);
    CHECK(rc2 == rc);
    if (rc2 == SPSP_OK) { report->assign(text, len); spsp_free(text); }
    free(rec); free(rp); free(np); free(parent); free(ref);
    return rc;
}

int main() {
    using namespace spsp;
    const uint32_t NONE = SPSP_TAXONOMY_NONE;
    static_assert(sizeof(spsp_taxonomy_record) == 40, "the record is 40 bytes");
    // the plan: the constants of spsp_internal.h, any pointer NULL, and its refusals
    uint32_t small = 0, nodes = 0, in_lds = 7, cut = 0;
    CHECK(spsp_taxonomy_plan_host(1, &small, &nodes, &in_lds, &cut) == SPSP_OK && small == kTxSmallHits && nodes == kTxLdsNodes && in_lds == 1 && cut == kTxListCut);
    CHECK(spsp_taxonomy_plan_host(kTxLdsNodes, nullptr, nullptr, &in_lds, nullptr) == SPSP_OK && in_lds == 1);
    CHECK(spsp_taxonomy_plan_host(kTxLdsNodes + 1, nullptr, nullptr, &in_lds, nullptr) == SPSP_OK && in_lds == 0);
    CHECK(spsp_taxonomy_plan_host(kTxMaxNodes, nullptr, nullptr, nullptr, nullptr) == SPSP_OK);
    CHECK((size_t)kTxLdsNodes * 4 + kTxLargeFixedLds <= kAcLdsBytes && kTxSmallHits * 4 == 4096);
    CHECK(spsp_taxonomy_plan_host(0, &small, &nodes, &in_lds, &cut) == SPSP_ERR_ARG && spsp_taxonomy_plan_host(kTxMaxNodes + 1, nullptr, nullptr, nullptr, nullptr) == SPSP_ERR_ARG);
    CHECK(taxonomy_check_args(1, 0, 1) == SPSP_OK && taxonomy_check_args(0xffffffffu, 1000000, 1000000) == SPSP_OK);
    CHECK(taxonomy_check_args(0, 0, 1) == SPSP_ERR_ARG && taxonomy_check_args(1, 2, 1) == SPSP_ERR_ARG && taxonomy_check_args(1, 0, 0) == SPSP_ERR_ARG);
    CHECK(taxonomy_check_args(1, 0, 1000001) == SPSP_ERR_ARG);

    // the parser: numbering by first appearance, one name under two parents, an inner node, an empty line, blanks, "\r\n", no final newline
    const Parsed P = parse("B;S;Se\nB;E;Ec\n\nB;E\n B ; E ; Ea \nZ;E\r\nB;S", 7);
    CHECK(P.rc == SPSP_OK && P.T == 9);
    CHECK(P.names == (std::vector<std::string>{"root", "B", "S", "Se", "E", "Ec", "Ea", "Z", "E"}));
    CHECK(P.parent == (std::vector<uint32_t>{0, 0, 1, 2, 1, 4, 4, 0, 7}) && P.depth == (std::vector<uint32_t>{0, 1, 2, 3, 2, 3, 3, 1, 2}));
    CHECK(P.size == (std::vector<uint32_t>{9, 6, 2, 1, 3, 1, 1, 2, 1}) && P.ref_node == (std::vector<uint32_t>{3, 5, 0, 4, 6, 8, 2}));
    CHECK(check(P.parent, P.ref_node) == SPSP_OK);
    CHECK(parse("\n\n", 2).T == 1 && parse("a", 1).T == 2);
    std::string deep;
    for (int i = 0; i < 32; ++i) deep += (i ? ";n" : "n") + std::to_string(i);
    CHECK(parse(deep + "\n", 1).T == 33 && parse(deep + "\n", 1).depth.back() == 32);
    struct { std::string text; uint32_t n; const char* line; } refused[] = {{deep + ";n32\n", 1, "line 1"}, {"a\nb,c\n", 2, "line 2"}, {"a\nb\n\"c\"\n", 3, "line 3"},
        {"a;;b\n", 1, "line 1"}, {"a;\n", 1, "line 1"}, {";a\n", 1, "line 1"}, {"a\n \n;\n", 3, "line 3"}, {"a\nb\n", 3, "line 3"}, {"a\nb\nc\n", 2, "line 3"}, {"", 1, "line 1"},
        {"a\x01\n", 1, "line 1"}};
    for (const auto& c : refused) { CHECK(parse(c.text, c.n).rc == SPSP_ERR_FORMAT); CHECK(strstr(spsp_last_error(), c.line) != nullptr); }
    CHECK(parse("a\n", 0).rc == SPSP_ERR_ARG && parse("a\n", 65536).rc == SPSP_ERR_ARG);
    uint32_t T = 0, ref1 = 0;
    CHECK(spsp_taxonomy_lineages_host("a\n", 2, 1, &ref1, nullptr, nullptr, nullptr, nullptr, nullptr, &T) == SPSP_OK && T == 2 && ref1 == 1);   // (every array NULL)
    CHECK(spsp_taxonomy_lineages_host(nullptr, 2, 1, &ref1, nullptr, nullptr, nullptr, nullptr, nullptr, &T) == SPSP_ERR_ARG);
    {   // many nodes: 3 000 references on private chains of 20 names
        std::string big;
        for (int j = 0; j < 3000; ++j) { for (int i = 0; i < 20; ++i) big += (i ? ";r" : "r") + std::to_string(j) + "_" + std::to_string(i); big += '\n'; }
        const Parsed Q = parse(big, 3000);
        CHECK(Q.rc == SPSP_OK && Q.T == 60001 && Q.ref_node.back() == 60000 && Q.size[0] == 60001 && check(Q.parent, Q.ref_node) == SPSP_OK);
    }

    // the check on arrays that break each condition in turn
    std::vector<uint32_t> chain(33);
    for (uint32_t t = 0; t < 33; ++t) chain[t] = t ? t - 1 : 0;
    CHECK(check(chain, {32}) == SPSP_OK && check({0}, {0, 0, 0}) == SPSP_OK);
    std::vector<uint32_t> deeper = chain;
    deeper.push_back(32);
    CHECK(check(deeper, {0}) == SPSP_ERR_ARG);                                           // depth 33
    CHECK(check({1, 0}, {0}) == SPSP_ERR_ARG && check({0, 1}, {0}) == SPSP_ERR_ARG && check({0, 0, 3, 1}, {0}) == SPSP_ERR_ARG);
    CHECK(check({0, 0, 1}, {3}) == SPSP_ERR_ARG && check({0, 0, 1}, {0, 2, 3}) == SPSP_ERR_ARG);
    CHECK(check({0, 0, 0, 1}, {0}) == SPSP_ERR_ARG && strstr(spsp_last_error(), "preorder") != nullptr);   // parent[t] < t holds
    CHECK(check({0, 0, 1, 0, 2}, {0}) == SPSP_ERR_ARG && check({}, {0}) == SPSP_ERR_ARG && check({0}, {}) == SPSP_ERR_ARG);
    CHECK(spsp_taxonomy_check_host(nullptr, 1, &ref1, 1) == SPSP_ERR_ARG);

    // the writers, over root 0 > B 1 > E 2 > {Ec 3, Ea 4}, B > S 5 > Se 6, Z 7; references at every node, two at Ec
    const Parsed H = parse("\nB\nB;E\nB;E;Ec\nB;E;Ea\nB;S\nB;S;Se\nZ\nB;E;Ec\n", 9);
    CHECK(H.rc == SPSP_OK && H.T == 8);
    std::string csv, report;
    const std::vector<Row> rows = {{5000, 16, 13, 2, 2, 6, 8, 2, 2}, {12, 0, 0, NONE, NONE, 0, 0, 0, 0}, {150, 16, 13, NONE, 2, 6, 0, 0, 2}, {40, 9, 9, 0, 0, 3, 9, 0, 3},
                                   {(1ull << 40) + 7, 7, 7, 6, 6, 7, 7, 7, 1}, {31, 5, 4, 1, 3, 3, 4, 1, 1}};
    CHECK(write_both(rows, H, 6, &csv, &report) == SPSP_OK);
    CHECK(csv == "record,name,length,keys,hit_keys,taxon,depth,lineage,score,clade,direct,f_clade,winners\n"
                 "0,rec0,5000,16,13,2,2,B;E,6,8,2,0.5,2\n1,rec1,12,0,0,,,,0,0,0,0,0\n2,rec2,150,16,13,,,,6,0,0,0,2\n3,rec3,40,9,9,0,0,,3,9,0,1,3\n"
                 "4,rec4,1099511627783,7,7,6,3,B;S;Se,7,7,7,1,1\n5,rec5,31,5,4,1,1,B,3,4,1,0.8,1\n");
    CHECK(report == "taxon,depth,name,lineage,references,records_clade,records_direct,bases_clade,bases_direct\n"
                    "0,0,root,,1,4,1,1099511632854,40\n1,1,B,B,1,3,1,1099511632814,31\n2,2,E,B;E,1,1,1,5000,5000\n3,3,Ec,B;E;Ec,2,0,0,0,0\n4,3,Ea,B;E;Ea,1,0,0,0,0\n"
                    "5,2,S,B;S,1,1,0,1099511627783,0\n6,3,Se,B;S;Se,1,1,1,1099511627783,1099511627783\n7,1,Z,Z,1,0,0,0,0\n,,unclassified,,0,2,2,162,162\n");
    CHECK(write_both({{1, 3, 3, 2, 2, 3, 1, 1, 1}}, H, 3, &csv, &report) == SPSP_OK && csv.find(",0.333,1\n") != std::string::npos);
    CHECK(write_both({}, H, 6, &csv, &report) == SPSP_OK && csv == "record,name,length,keys,hit_keys,taxon,depth,lineage,score,clade,direct,f_clade,winners\n");
    CHECK(report.find("\n,,unclassified,,0,0,0,0,0\n") != std::string::npos);
    CHECK(write_both({{9, 3, 3, 0, 0, 3, 3, 3, 1}}, parse("\n", 1), 6, &csv, &report) == SPSP_OK && csv.find("\n0,rec0,9,3,3,0,0,,3,3,3,1,1\n") != std::string::npos);   // T = 1
    CHECK(write_both({{1, 1, 1, 7, 7, 1, 1, 1, 1}}, H, 6, &csv, &report) == SPSP_OK);      // the tree's last node
    // rows that contradict themselves, each refused by both writers with the record named
    const std::vector<Row> bad = {{1, 6, 7, 2, 2, 3, 5, 1, 1},       // hit_keys > keys
                                  {1, 9, 5, 2, 2, 3, 6, 1, 1},       // clade > hit_keys
                                  {1, 9, 5, 2, 2, 3, 4, 5, 1},       // direct > clade
                                  {1, 9, 5, 2, 2, 6, 4, 1, 1},       // score > hit_keys
                                  {1, 9, 5, 8, 8, 3, 4, 1, 1},       // node >= T and not none
                                  {1, 9, 5, 0xfffffffeu, 2, 3, 4, 1, 1},
                                  {1, 9, 5, 2, 5, 3, 4, 1, 1},       // node E is no ancestor of start S
                                  {1, 9, 5, 3, 2, 3, 4, 1, 1},       // node Ec below start E
                                  {1, 9, 5, 2, NONE, 3, 4, 1, 1},    // a call without a start
                                  {1, 9, 5, 2, 0xfffffff0u, 3, 4, 1, 1},
                                  {1, 9, 5, 2, 2, 3, 4, 1, 0}};      // winners = 0 with hit keys
    for (const Row& b : bad) {
        CHECK(write_both({rows[0], b}, H, 6, &csv, &report) == SPSP_ERR_ARG && csv.empty() && report.empty());
        CHECK(strstr(spsp_last_error(), "record 1") != nullptr);
    }
    Parsed broken = H;
    broken.parent = {0, 0, 0, 1, 1, 1, 1, 1};                                             // no preorder
    CHECK(write_both(rows, broken, 6, &csv, &report) == SPSP_ERR_ARG);
    char* text = nullptr; uint64_t len = 0;
    CHECK(spsp_taxonomy_csv_host(nullptr, 1, nullptr, H.parent.data(), H.T, nullptr, 6, &text, &len) == SPSP_ERR_ARG);
    CHECK(spsp_taxonomy_report_csv_host(nullptr, 0, H.parent.data(), H.T, nullptr, H.ref_node.data(), 9, nullptr, &len) == SPSP_ERR_ARG);
    printf("taxonomy_asan: ok\n");
    return 0;
}
