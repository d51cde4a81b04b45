// The host half of the depth pass -- the plan (spsp_depth_plan_host) and the CSV writer with its refusals (spsp_depth_csv_host) --
// driven on the CPU by a program of its own, so that it can be built with AddressSanitizer + UBSan (run.sh).  No device, no Python.
// Every buffer handed in has its exact size on the heap: a read behind rows[n_ref - 1], or behind the last name, is ASan's to find.
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

// keys found sum median max | the unique five
struct Row { uint32_t keys, found; uint64_t sum; uint32_t median, max, ukeys, ufound; uint64_t usum; uint32_t umedian, umax; };

// the writer on arrays of exactly their sizes: -> its rc, the text
static int write(const std::vector<Row>& rows, int precision, std::string* csv) {
    const size_t n = rows.size();
    spsp_depth_row* r = (spsp_depth_row*)malloc((n ? n : 1) * sizeof(spsp_depth_row));
    std::vector<std::string> names(n);
    const char** np = (const char**)malloc((n ? n : 1) * sizeof(char*));
    for (size_t j = 0; j < n; ++j) {
        r[j].keys = rows[j].keys; r[j].found = rows[j].found; r[j].sum = rows[j].sum; r[j].median = rows[j].median; r[j].max = rows[j].max;
        r[j].unique_keys = rows[j].ukeys; r[j].unique_found = rows[j].ufound; r[j].unique_sum = rows[j].usum; r[j].unique_median = rows[j].umedian;
        r[j].unique_max = rows[j].umax;
        names[j] = "ref " + std::to_string(j) + ".gz"; np[j] = names[j].c_str();
    }
    char* text = nullptr; uint64_t len = 0;
    const int rc = spsp_depth_csv_host(n ? r : nullptr, n ? np : nullptr, (uint32_t)n, precision, &text, &len);
    csv->clear();
    if (rc == SPSP_OK) { csv->assign(text, len); spsp_free(text); }
    else CHECK(text == nullptr);
    free(r); free(np);
    return rc;
}

int main() {
    using namespace spsp;
    static_assert(sizeof(spsp_depth_row) == 48 && sizeof(spsp_depth_totals) == 24, "the rows' sizes are part of the interface");
    uint32_t bins = 0;
    CHECK(spsp_depth_plan_host(&bins) == SPSP_OK && bins == kDpBins && bins % kDpThreads == 0);
    CHECK(spsp_depth_plan_host(nullptr) == SPSP_ERR_ARG);

    const std::string header = "reference,keys,found,f_found,median,mean,max,unique_keys,unique_found,f_unique_found,unique_median,unique_mean,unique_max\n";
    std::string csv;
    const Row good{6, 5, 17, 3, 9, 2, 1, 9, 9, 9};
    const std::vector<Row> rows = {good, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {7, 0, 0, 0, 0, 7, 0, 0, 0, 0},
                                   {3, 3, 3ull * 0xffffffffull - 5, 1u << 31, 0xffffffffu, 3, 3, 3ull * 0xffffffffull - 5, 1u << 31, 0xffffffffu}, {3, 3, 7, 2, 3, 0, 0, 0, 0, 0}};
    CHECK(write(rows, 6, &csv) == SPSP_OK);
    CHECK(csv == header + "ref 0.gz,6,5,0.833333,3,3.4,9,2,1,0.5,9,9,9\nref 1.gz,0,0,0,0,0,0,0,0,0,0,0,0\nref 2.gz,7,0,0,0,0,0,7,0,0,0,0,0\n"
                          "ref 3.gz,3,3,1,2147483648,4.29497e+09,4294967295,3,3,1,2147483648,4.29497e+09,4294967295\nref 4.gz,3,3,1,2,2.33333,3,0,0,0,0,0,0\n");
    CHECK(write(rows, 3, &csv) == SPSP_OK && csv.find("ref 0.gz,6,5,0.833,3,3.4,9,") != std::string::npos && csv.find(",2.33,3,0,") != std::string::npos);
    CHECK(write({}, 6, &csv) == SPSP_OK && csv == header);
    CHECK(write(std::vector<Row>(65535, good), 6, &csv) == SPSP_OK && csv.find("ref 65534.gz,6,5,") != std::string::npos);
    // rows that contradict themselves, each refused with the reference named
    const std::vector<Row> bad = {{6, 7, 17, 3, 9, 2, 1, 9, 9, 9},       // found > keys
                                  {6, 5, 17, 3, 9, 7, 1, 9, 9, 9},       // unique_keys > keys
                                  {6, 5, 17, 3, 9, 2, 3, 9, 3, 3},       // unique_found > unique_keys
                                  {6, 1, 9, 9, 9, 2, 2, 2, 1, 1},        // unique_found > found
                                  {6, 5, 17, 10, 9, 2, 1, 9, 9, 9},      // median > max
                                  {6, 1, 3, 3, 4, 2, 0, 0, 0, 0},        // max > sum
                                  {6, 0, 3, 0, 0, 2, 0, 0, 0, 0},        // found == 0 with a sum
                                  {6, 0, 0, 0, 1, 2, 0, 0, 0, 0},        // ... with a max
                                  {6, 5, 17, 0, 9, 2, 1, 9, 9, 9},       // found > 0 with median == 0
                                  {6, 5, 4, 1, 1, 2, 0, 0, 0, 0},        // sum < found
                                  {6, 5, 46, 3, 9, 2, 1, 9, 9, 9},       // sum > found * max
                                  {6, 5, 17, 3, 9, 2, 1, 9, 10, 9},      // the unique five: median > max
                                  {6, 5, 17, 3, 9, 2, 1, 8, 9, 9},       // ... max > sum
                                  {6, 5, 17, 3, 9, 2, 0, 0, 0, 2},       // ... nothing found, and a max
                                  {6, 5, 17, 3, 9, 2, 2, 9, 0, 9},       // ... found with median == 0
                                  {6, 5, 17, 3, 9, 2, 2, 1, 1, 1},       // ... sum < found
                                  {6, 5, 17, 3, 9, 2, 2, 19, 9, 9},      // ... sum > found * max
                                  {6, 5, 17, 3, 9, 2, 2, 18, 9, 9},      // unique_sum > sum
                                  {0xffffffffu, 0xffffffffu, 0xffffffffull * 0xffffffffull + 1, 0xffffffffu, 0xffffffffu, 0, 0, 0, 0, 0}};   // found * max in 64 bits
    for (const Row& b : bad) {
        CHECK(write({good, b}, 6, &csv) == SPSP_ERR_ARG && csv.empty());
        CHECK(strstr(spsp_last_error(), "reference 1") != nullptr);
    }
    CHECK(write({{0xffffffffu, 0xffffffffu, 0xffffffffull * 0xffffffffull, 0xffffffffu, 0xffffffffu, 0, 0, 0, 0, 0}}, 6, &csv) == SPSP_OK);
    char* text = nullptr; uint64_t len = 0;
    CHECK(spsp_depth_csv_host(nullptr, nullptr, 1, 6, &text, &len) == SPSP_ERR_ARG);
    CHECK(spsp_depth_csv_host(nullptr, nullptr, 0, 6, nullptr, &len) == SPSP_ERR_ARG);
    printf("depth_asan: ok\n");
    return 0;
}
