// The host half of the record file drivers -- the records' names as the host reads them (record_names_host), the batches' bounds
// (records_batch_bounds), the one file writer of the extraction and the split (write_bytes) and the handing out of several row
// arrays (give_rows_all) -- driven on the CPU by a program of its own, so that it can be built with AddressSanitizer + UBSan
// (run.sh).  No device, no Python.  Every text handed in has its exact size on the heap and no 0 byte behind it: a read behind
// text[n - 1] is ASan's to find.
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

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

using namespace spsp;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, spsp_last_error()); exit(1); } \
    } while (0)

typedef std::vector<std::string> Names;

// the names of a text held in a heap block of exactly its size
static Names names_of(const std::string& text, bool fastq) {
    uint8_t* p = (uint8_t*)malloc(text.size() ? text.size() : 1);
    if (!text.empty()) memcpy(p, text.data(), text.size());
    Names names;
    record_names_host(p, text.size(), fastq, &names);
    free(p);
    return names;
}

static void names() {
    CHECK((names_of(">a\nAC\n>b x\nGG\nTT\n>c\ty\nT\n", false) == Names{"a", "b", "c"}));
    CHECK((names_of(">a\r\nAC\r\n>b x\r\nGG\r\n", false) == Names{"a", "b"}));                  // CRLF: the '\r' ends the word
    CHECK((names_of(">\nAC\n> x\nGG\n>\r\nT\n", false) == Names{"", "", ""}));                   // empty headers
    CHECK((names_of(">a\nAC\n>b\nGG", false) == Names{"a", "b"}));                               // no final newline
    CHECK((names_of(">a\nAC\n>b", false) == Names{"a", "b"}));                                   // ... and a header as the last line
    CHECK((names_of(">a\nAC\n\n\n\n", false) == Names{"a"}));                                    // trailing blank lines
    CHECK((names_of("AC\n>a\nAC\n", false) == Names{"a"}));                                      // bases in front of the first header: no name
    CHECK((names_of(">", false) == Names{""}));
    CHECK(names_of("", false).empty() && names_of("", true).empty());                            // the empty text
    CHECK(names_of("\n\n", false).empty() && names_of("\n\n", true).empty());
    CHECK((names_of("@r1 d\nACGT\n+\nIIII\n@r2\nAC\n+\nII\n", true) == Names{"r1", "r2"}));
    CHECK((names_of("@r1\nAC\n+\n@I\n@r2\nAC\n+\n>I\n", true) == Names{"r1", "r2"}));             // '@' and '>' in front of a quality line
    CHECK((names_of("@r1\r\nAC\r\n+\r\nII\r\n@r2\tz\r\nAC\r\n+\r\nII\r\n", true) == Names{"r1", "r2"}));
    CHECK((names_of("@\nAC\n+\nII\n@ x\nAC\n+\nII\n", true) == Names{"", ""}));
    CHECK((names_of("@r1\nAC\n+\nII\n@r2\nAC\n+\nII", true) == Names{"r1", "r2"}));               // no final newline
    CHECK((names_of("@r1\nAC\n+\nII\n@r2\nAC\n+\nII\n\n\r\n\n", true) == Names{"r1", "r2"}));     // trailing blank lines: no fifth line
    CHECK((names_of("@r1\nAC\n+\nII\n@r2", true) == Names{"r1", "r2"}));                          // a content that ends in a header
    CHECK((names_of("@", true) == Names{""}));
}

static void bounds() {
    typedef std::vector<uint32_t> B;
    CHECK((records_batch_bounds(0) == B{0}));                                                    // no batch
    CHECK((records_batch_bounds(1) == B{0, 1}));
    CHECK((records_batch_bounds(65535) == B{0, 65535}));
    CHECK((records_batch_bounds(65536) == B{0, 65535, 65536}));
    CHECK((records_batch_bounds(131071) == B{0, 65535, 131070, 131071}));
    CHECK((records_batch_bounds(131070) == B{0, 65535, 131070}));
    const B top = records_batch_bounds(0xffffffffu);                                             // the counter does not wrap
    CHECK(top.size() == 65538 && top.back() == 0xffffffffu && top[top.size() - 2] == 65536u * 65535u);   // (65537 batches of 65 535: 2^32 - 1)
    for (size_t b = 0; b + 1 < top.size(); ++b) CHECK(top[b] < top[b + 1] && top[b + 1] - top[b] <= 65535);
}

static std::string slurp(const std::string& path, bool gz) {
    std::string out;
    char buf[4096];
    if (gz) {
        gzFile f = gzopen(path.c_str(), "rb");
        CHECK(f != nullptr);
        for (int n; (n = gzread(f, buf, sizeof buf)) > 0;) out.append(buf, (size_t)n);
        gzclose(f);
    } else {
        FILE* f = fopen(path.c_str(), "rb");
        CHECK(f != nullptr);
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) out.append(buf, n);
        fclose(f);
    }
    return out;
}

static void writes() {
    char dir[] = "/tmp/record_files_asan.XXXXXX";
    CHECK(mkdtemp(dir) != nullptr);
    const std::string root = dir;
    std::string big;
    for (int i = 0; i < 20000; ++i) big += ">r" + std::to_string(i) + "\nACGTTGCA\n";
    for (const std::string& text : {std::string(">a\nAC\n"), std::string(), big}) {
        uint8_t* p = (uint8_t*)malloc(text.size() ? text.size() : 1);
        if (!text.empty()) memcpy(p, text.data(), text.size());
        for (int gz = 0; gz < 2; ++gz) {
            const std::string path = root + (gz ? "/out.fa.gz" : "/out.fa");
            CHECK(write_bytes(path.c_str(), p, text.size(), gz) == SPSP_OK);
            CHECK(slurp(path, gz != 0) == text);
            if (!gz) { struct stat st; CHECK(stat(path.c_str(), &st) == 0 && (uint64_t)st.st_size == text.size()); }   // as it is: no byte more
            else if (!text.empty()) { const std::string raw = slurp(path, false); CHECK(raw.size() >= 2 && (uint8_t)raw[0] == 0x1f && (uint8_t)raw[1] == 0x8b); }
            CHECK(remove(path.c_str()) == 0);
        }
        const std::string nowhere = root + "/no such directory/out.fa";                          // an unwritable path, in both forms
        CHECK(write_bytes(nowhere.c_str(), p, text.size(), 0) == SPSP_ERR_IO);
        CHECK(std::string(spsp_last_error()) == "cannot write '" + nowhere + "'");
        CHECK(write_bytes(nowhere.c_str(), p, text.size(), 1) == SPSP_ERR_IO);
        CHECK(std::string(spsp_last_error()) == "cannot create '" + nowhere + "'");                // (spsp_write_gz_host's own text)
        free(p);
    }
    CHECK(rmdir(dir) == 0);
}

static void gifts() {
    const std::vector<uint32_t> a{1, 2, 3};
    const std::vector<uint64_t> b;
    void *pa = &pa, *pb = &pb;
    const RowsGift all[] = {{&pa, a.data(), a.size() * 4}, {nullptr, a.data(), a.size() * 4}, {&pb, b.data(), 0}};
    CHECK(give_rows_all(all, 3) == SPSP_OK && pa && pb && pa != (void*)&pa && pb != (void*)&pb);   // one byte for no rows: never NULL
    CHECK(memcmp(pa, a.data(), 12) == 0);
    free(pa); free(pb);
    CHECK(give_rows_all(all, 0) == SPSP_OK);
}

int main() {
    names();
    bounds();
    writes();
    gifts();
    printf("record_files_asan: ok\n");
    return 0;
}
