// The host half of the classification -- the plan (spsp_classify_plan_host) and the two CSV writers with their refusals
// (spsp_classify_csv_host, spsp_classify_summary_csv_host) -- driven on the CPU by a program of its own, so that it can be built
// with AddressSanitizer + UBSan (run.sh).  No device, no Python.  Every buffer handed in has its exact size on the heap: a read
// behind hits[n_records * top - 1], or behind the last name, is ASan's to find.
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

struct Row { uint64_t length; uint32_t keys, hit_keys, passing; std::vector<std::pair<uint32_t, uint32_t>> best; };

// both writers on arrays of exactly their sizes: -> rc of the first (the second must agree), the two texts
static int write_both(const std::vector<Row>& rows, uint32_t top, uint32_t n_ref, int precision, std::string* csv, std::string* summary) {
    const size_t n = rows.size();
    spsp_classify_record* rec = (spsp_classify_record*)malloc((n ? n : 1) * sizeof(spsp_classify_record));
    spsp_classify_hit* hit = (spsp_classify_hit*)calloc(n * top ? n * top : 1, sizeof(spsp_classify_hit));
    std::vector<std::string> rn(n), fn(n_ref);
    const char** rp = (const char**)malloc((n ? n : 1) * sizeof(char*));
    const char** fp = (const char**)malloc((n_ref ? n_ref : 1) * sizeof(char*));
    for (size_t r = 0; r < n; ++r) {
        rec[r].length = rows[r].length; rec[r].keys = rows[r].keys; rec[r].hit_keys = rows[r].hit_keys; rec[r].passing = rows[r].passing;
        rec[r].listed = (uint32_t)rows[r].best.size();
        for (size_t i = 0; i < rows[r].best.size() && i < top; ++i) { hit[r * top + i].reference = rows[r].best[i].first; hit[r * top + i].shared = rows[r].best[i].second; }
        rn[r] = "rec" + std::to_string(r); rp[r] = rn[r].c_str();
    }
    for (uint32_t j = 0; j < n_ref; ++j) { fn[j] = "ref " + std::to_string(j) + ".gz"; fp[j] = fn[j].c_str(); }
    char* text = nullptr; uint64_t len = 0;
    const int rc = spsp_classify_csv_host(n ? rec : nullptr, n ? hit : nullptr, n, rp, fp, n_ref, top, precision, &text, &len);
    csv->clear(); summary->clear();
    if (rc == SPSP_OK) { csv->assign(text, len); spsp_free(text); }
    text = nullptr; len = 0;
    const int rc2 = spsp_classify_summary_csv_host(n ? rec : nullptr, n ? hit : nullptr, n, fp, n_ref, top, &text, &len);
    CHECK(rc2 == rc);
    if (rc2 == SPSP_OK) { summary->assign(text, len); spsp_free(text); }
    free(rec); free(hit); free(rp); free(fp);
    return rc;
}

int main() {
    using namespace spsp;
    // the plan: the constants of spsp_internal.h, any pointer NULL, and its refusals
    uint32_t small = 0, refs = 0, in_lds = 7, cut = 0;
    CHECK(spsp_classify_plan_host(1, 1, &small, &refs, &in_lds, &cut) == SPSP_OK && small == kCfSmallWork && refs == kCfLdsRefs && in_lds == 1 && cut == kCfListCut);
    CHECK(spsp_classify_plan_host(kCfLdsRefs, 64, nullptr, nullptr, &in_lds, nullptr) == SPSP_OK && in_lds == 1);
    CHECK(spsp_classify_plan_host(kCfLdsRefs + 1, 64, nullptr, nullptr, &in_lds, nullptr) == SPSP_OK && in_lds == 0);
    CHECK(spsp_classify_plan_host(65535, 1, nullptr, nullptr, nullptr, nullptr) == SPSP_OK);
    CHECK((size_t)kCfLdsRefs * 4 + kCfLargeFixedLds <= kAcLdsBytes);
    CHECK(spsp_classify_plan_host(0, 1, &small, &refs, &in_lds, &cut) == SPSP_ERR_ARG && spsp_classify_plan_host(65536, 1, nullptr, nullptr, nullptr, nullptr) == SPSP_ERR_ARG);
    CHECK(spsp_classify_plan_host(5, 0, nullptr, nullptr, nullptr, nullptr) == SPSP_ERR_ARG && spsp_classify_plan_host(5, 65, nullptr, nullptr, nullptr, nullptr) == SPSP_ERR_ARG);
    CHECK(classify_check_args(1, 1, 0, 1) == SPSP_OK && classify_check_args(64, 0xffffffffu, 1000000, 1000000) == SPSP_OK);
    CHECK(classify_check_args(0, 1, 0, 1) == SPSP_ERR_ARG && classify_check_args(65, 1, 0, 1) == SPSP_ERR_ARG && classify_check_args(1, 0, 0, 1) == SPSP_ERR_ARG);
    CHECK(classify_check_args(1, 1, 2, 1) == SPSP_ERR_ARG && classify_check_args(1, 1, 0, 0) == SPSP_ERR_ARG && classify_check_args(1, 1, 0, 1000001) == SPSP_ERR_ARG);

    // the writers
    std::string csv, summary;
    const std::vector<Row> rows = {{5000, 6, 5, 3, {{0, 4}, {3, 4}}}, {12, 0, 0, 0, {}}, {150, 2, 0, 0, {}}, {40, 1, 1, 1, {{2, 1}}}, {(1ull << 40) + 7, 7, 7, 5, {{1, 7}, {0, 3}}}};
    CHECK(write_both(rows, 2, 4, 6, &csv, &summary) == SPSP_OK);
    CHECK(csv == "record,name,length,keys,hit_keys,rank,match,shared,f_shared,passing\n"
                 "0,rec0,5000,6,5,1,ref 0.gz,4,0.666667,3\n0,rec0,5000,6,5,2,ref 3.gz,4,0.666667,3\n1,rec1,12,0,0,0,,0,0,0\n2,rec2,150,2,0,0,,0,0,0\n"
                 "3,rec3,40,1,1,1,ref 2.gz,1,1,1\n4,rec4,1099511627783,7,7,1,ref 1.gz,7,1,5\n4,rec4,1099511627783,7,7,2,ref 0.gz,3,0.428571,5\n");
    CHECK(summary == "reference,records_best,bases_best,keys_best,records_listed\nref 0.gz,1,5000,4,2\nref 1.gz,1,1099511627783,7,1\nref 2.gz,1,40,1,1\n"
                     "ref 3.gz,0,0,0,1\nunclassified,2,162,0,0\n");
    CHECK(write_both(rows, 2, 4, 3, &csv, &summary) == SPSP_OK && csv.find(",0.429,5\n") != std::string::npos);
    CHECK(write_both({}, 1, 1, 6, &csv, &summary) == SPSP_OK && csv == "record,name,length,keys,hit_keys,rank,match,shared,f_shared,passing\n");
    CHECK(summary == "reference,records_best,bases_best,keys_best,records_listed\nref 0.gz,0,0,0,0\nunclassified,0,0,0,0\n");
    // top = 64 and every slot taken; top = 1 with the last record's hit in the array's last slot
    {
        Row full{1000, 100, 100, 70, {}};
        for (uint32_t i = 0; i < 64; ++i) full.best.push_back({i, 100 - i});
        CHECK(write_both({full, full}, 64, 65535, 6, &csv, &summary) == SPSP_OK);
        CHECK(write_both({{1, 1, 1, 1, {{65534, 1}}}}, 1, 65535, 6, &csv, &summary) == SPSP_OK && csv.find("ref 65534.gz") != std::string::npos);
    }
    // rows that contradict themselves, each refused by both writers with the record named
    const std::vector<Row> bad = {{1, 6, 5, 1, {{0, 4}, {3, 4}}},    // listed > passing
                                  {1, 6, 7, 3, {{0, 4}}},            // hit_keys > keys
                                  {1, 6, 3, 3, {{0, 4}}},            // shared > hit_keys
                                  {1, 6, 5, 3, {{3, 4}, {0, 4}}},    // equal shared, the higher reference first
                                  {1, 6, 5, 3, {{0, 3}, {3, 4}}},    // shared rising
                                  {1, 6, 5, 3, {{0, 4}, {0, 4}}},    // one reference twice
                                  {1, 6, 5, 3, {{4, 4}}},            // reference >= R
                                  {1, 6, 5, 3, {{0, 0}}},            // a listed match that shares nothing
                                  {1, 6, 5, 9, {{0, 4}, {1, 3}, {2, 2}}}};   // listed > top
    for (const Row& b : bad) {
        CHECK(write_both({rows[3], b}, 2, 4, 6, &csv, &summary) == SPSP_ERR_ARG && csv.empty() && summary.empty());
        CHECK(strstr(spsp_last_error(), "record 1") != nullptr);
    }
    CHECK(write_both(rows, 0, 4, 6, &csv, &summary) == SPSP_ERR_ARG && write_both(rows, 65, 4, 6, &csv, &summary) == SPSP_ERR_ARG);
    CHECK(write_both(rows, 2, 0, 6, &csv, &summary) == SPSP_ERR_ARG);
    char* text = nullptr; uint64_t len = 0;
    CHECK(spsp_classify_csv_host(nullptr, nullptr, 1, nullptr, nullptr, 1, 1, 6, &text, &len) == SPSP_ERR_ARG);
    CHECK(spsp_classify_summary_csv_host(nullptr, nullptr, 0, nullptr, 1, 1, nullptr, &len) == SPSP_ERR_ARG);
    printf("classify_asan: ok\n");
    return 0;
}
