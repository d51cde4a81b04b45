// The host half of the profile pass -- the CSV writer with its refusals (spsp_profile_csv_host) -- driven on the CPU by a program
// of its own, so that it can be built with AddressSanitizer + UBSan (run.sh).  No device, no Python.  Every buffer handed in has
// its exact size on the heap: a read behind rows[n_rows - 1], or behind the last name, is ASan's to find.
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

struct Row { uint32_t reference, keys, found, assigned; uint64_t sum; uint32_t median, max, remaining; };
struct Totals { uint32_t found_keys; uint64_t found_sum; };

// the writer on arrays of exactly their sizes: -> its rc, the text
static int write(const std::vector<Row>& rows, Totals t, uint32_t n_ref, int precision, std::string* csv) {
    const size_t n = rows.size();
    spsp_profile_row* r = (spsp_profile_row*)malloc((n ? n : 1) * sizeof(spsp_profile_row));
    spsp_profile_totals* tot = (spsp_profile_totals*)malloc(sizeof(spsp_profile_totals));
    std::vector<std::string> names(n_ref);
    const char** np = (const char**)malloc((n_ref ? n_ref : 1) * sizeof(char*));
    tot->found_keys = t.found_keys; tot->found_sum = t.found_sum; tot->assigned_keys = 0; tot->assigned_sum = 0;
    for (size_t i = 0; i < n; ++i) {
        r[i].reference = rows[i].reference; r[i].keys = rows[i].keys; r[i].found = rows[i].found; r[i].assigned = rows[i].assigned; r[i].sum = rows[i].sum;
        r[i].median = rows[i].median; r[i].max = rows[i].max; r[i].remaining = rows[i].remaining; r[i].reserved = 0;
        tot->assigned_keys += rows[i].assigned; tot->assigned_sum += rows[i].sum;
    }
    for (uint32_t j = 0; j < n_ref; ++j) { names[j] = "ref " + std::to_string(j) + ".gz"; np[j] = names[j].c_str(); }
    char* text = nullptr; uint64_t len = 0;
    const int rc = spsp_profile_csv_host(n ? r : nullptr, n, tot, n_ref ? np : nullptr, n_ref, precision, &text, &len);
    csv->clear();
    if (rc == SPSP_OK) { csv->assign(text, len); spsp_free(text); }
    else CHECK(text == nullptr);
    free(r); free(tot); free(np);
    return rc;
}

int main() {
    static_assert(sizeof(spsp_profile_row) == 40 && sizeof(spsp_profile_totals) == 24, "the rows' sizes are part of the interface");
    const std::string header = "rank,reference,keys,found,f_found,assigned,f_assigned,median,mean,max,f_weighted,remaining\n";
    std::string csv;
    const Totals totals{20, 100};
    const std::vector<Row> good = {{2, 10, 9, 8, 40, 4, 9, 12}, {0, 12, 8, 8, 30, 3, 7, 4}, {1, 5, 4, 3, 3, 1, 1, 1}};
    CHECK(write(good, totals, 3, 6, &csv) == SPSP_OK);
    CHECK(csv == header + "1,ref 2.gz,10,9,0.9,8,0.4,4,5,9,0.4,12\n2,ref 0.gz,12,8,0.666667,8,0.4,3,3.75,7,0.3,4\n3,ref 1.gz,5,4,0.8,3,0.15,1,1,1,0.03,1\n");
    CHECK(write(good, totals, 3, 3, &csv) == SPSP_OK && csv.find("2,ref 0.gz,12,8,0.667,8,") != std::string::npos);
    CHECK(write(good, totals, 70000, 6, &csv) == SPSP_OK);                                   // more references than rows
    CHECK(write({}, {0, 0}, 3, 6, &csv) == SPSP_OK && csv == header);
    CHECK(write({}, {0, 0}, 0, 6, &csv) == SPSP_OK && csv == header);
    // the largest values: assigned * max in 64 bits
    CHECK(write({{0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffull * 0xffffffffull, 1u << 31, 0xffffffffu, 0}}, {0xffffffffu, 0xffffffffull * 0xffffffffull}, 1, 6, &csv) == SPSP_OK);
    CHECK(csv == header + "1,ref 0.gz,4294967295,4294967295,1,4294967295,1,2147483648,4.29497e+09,4294967295,1,0\n");
    CHECK(write({{0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffull * 0xffffffffull + 1, 1u << 31, 0xffffffffu, 0}}, {0xffffffffu, ~0ull}, 1, 6, &csv) == SPSP_ERR_ARG);
    // 65535 rows of one key each
    {
        std::vector<Row> many;
        for (uint32_t j = 0; j < 65535; ++j) many.push_back({65534 - j, 1, 1, 1, 2, 2, 2, 65534 - j});
        CHECK(write(many, {65535, 131070}, 65535, 6, &csv) == SPSP_OK && csv.find("65535,ref 0.gz,1,1,1,1,") != std::string::npos);
    }
    // rows that contradict the rule, each refused with the rank named: in the place of the second row
    const std::vector<Row> bad = {{0, 12, 9, 9, 30, 3, 7, 3},        // assigned increases from one row to the next
                                  {0, 12, 8, 0, 0, 0, 0, 12},        // nothing assigned
                                  {0, 12, 7, 8, 30, 3, 7, 4},        // assigned > found
                                  {0, 7, 8, 8, 30, 3, 7, 4},         // found > keys
                                  {2, 12, 8, 8, 30, 3, 7, 4},        // a reference twice
                                  {3, 12, 8, 8, 30, 3, 7, 4},        // a reference the index does not have
                                  {0xffffffffu, 12, 8, 8, 30, 3, 7, 4},
                                  {0, 12, 8, 8, 30, 3, 7, 5},        // remaining is not the last remaining less assigned
                                  {0, 12, 8, 8, 30, 3, 7, 3},
                                  {0, 13, 13, 13, 30, 3, 7, 0xffffffffu},   // more assigned than were left
                                  {0, 12, 8, 8, 7, 1, 1, 4},         // sum < assigned
                                  {0, 12, 8, 8, 57, 3, 7, 4},        // sum > assigned * max
                                  {0, 12, 8, 8, 30, 0, 7, 4},        // median == 0
                                  {0, 12, 8, 8, 30, 8, 7, 4}};       // median > max
    for (const Row& b : bad) {
        CHECK(write({good[0], b, good[2]}, totals, 3, 6, &csv) == SPSP_ERR_ARG && csv.empty());
        CHECK(strstr(spsp_last_error(), "rank 2") != nullptr);
    }
    CHECK(write(good, {21, 100}, 3, 6, &csv) == SPSP_ERR_ARG && strstr(spsp_last_error(), "rank 1") != nullptr);   // remaining_0 is |F|
    CHECK(write(good, totals, 2, 6, &csv) == SPSP_ERR_ARG && strstr(spsp_last_error(), "rank 3") != nullptr);      // more rows than references
    char* text = nullptr; uint64_t len = 0;
    spsp_profile_totals t{};
    CHECK(spsp_profile_csv_host(nullptr, 1, &t, nullptr, 1, 6, &text, &len) == SPSP_ERR_ARG);
    CHECK(spsp_profile_csv_host(nullptr, 0, nullptr, nullptr, 0, 6, &text, &len) == SPSP_ERR_ARG);
    CHECK(spsp_profile_csv_host(nullptr, 0, &t, nullptr, 0, 6, nullptr, &len) == SPSP_ERR_ARG);
    printf("profile_asan: ok\n");
    return 0;
}
