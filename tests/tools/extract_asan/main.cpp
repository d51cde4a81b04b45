// The host half of the extraction -- the records' starts (spsp_records_extents_host), the extraction (spsp_records_extract_host),
// the two flag functions with their refusals (spsp_extract_flags_classify_host, spsp_extract_flags_taxonomy_host,
// spsp_extract_word_check_host) and the plan -- driven on the CPU by a program of its own, so that it can be built with
// AddressSanitizer + UBSan (run.sh).  No device, no Python.  Every buffer handed in has its exact size on the heap and no 0 byte
// behind a text: a read behind text[n - 1], keep[n_rec - 1], hits[n * top - 1] or size[T - 1] is ASan's to find.
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

// a text in a heap block of exactly its size
struct Exact {
    uint8_t* p;
    uint64_t n;
    explicit Exact(const std::string& s) : p((uint8_t*)malloc(s.size() ? s.size() : 1)), n(s.size()) { memcpy(p, s.data(), s.size()); }
    ~Exact() { free(p); }
};

// the starts of a text, or the call's refusal
static int extents(const std::string& text, std::vector<uint64_t>* begin) {
    Exact t(text);
    uint64_t* b = nullptr; uint32_t n_rec = 0;
    const int rc = spsp_records_extents_host(t.n ? t.p : nullptr, t.n, &b, &n_rec);
    begin->clear();
    if (rc == SPSP_OK) { begin->assign(b, b + n_rec + 1); spsp_free(b); }
    else CHECK(b == nullptr && n_rec == 0);
    return rc;
}

static std::string extract(const std::string& text, const std::vector<uint8_t>& keep, uint64_t* n_kept) {
    std::vector<uint64_t> begin;
    CHECK(extents(text, &begin) == SPSP_OK && begin.size() == keep.size() + 1);
    Exact t(text);
    uint64_t* b = (uint64_t*)malloc(begin.size() * 8);
    memcpy(b, begin.data(), begin.size() * 8);
    uint8_t* k = (uint8_t*)malloc(keep.size() ? keep.size() : 1);
    memcpy(k, keep.data(), keep.size());
    uint8_t* out = nullptr; uint64_t n_out = 0;
    CHECK(spsp_records_extract_host(t.n ? t.p : nullptr, t.n, b, (uint32_t)keep.size(), k, &out, &n_out, n_kept) == SPSP_OK);
    std::string got((const char*)out, (size_t)n_out);
    spsp_free(out); free(b); free(k);
    return got;
}

static std::string keep_all(const std::string& text) {
    std::vector<uint64_t> begin;
    CHECK(extents(text, &begin) == SPSP_OK);
    uint64_t kept = 0;
    const std::string got = extract(text, std::vector<uint8_t>(begin.size() - 1, 1), &kept);
    CHECK(kept == begin.size() - 1);
    return got;
}

int main() {
    using V = std::vector<uint64_t>;
    V b;
    uint32_t tile = 0, stretch = 0;
    CHECK(spsp_extract_plan_host(&tile, &stretch) == SPSP_OK && tile == spsp::kExTile && stretch == spsp::kExStretch);
    CHECK(spsp_extract_plan_host(nullptr, nullptr) == SPSP_OK);

    // FASTA: the empty text, one-byte records, line 0 whatever it holds, '>' inside a line, 0xFF, "\r\n", no final newline
    CHECK(extents("", &b) == SPSP_OK && b == V({0, 0}));
    CHECK(extents("\n", &b) == SPSP_OK && b == V({0, 1}));
    CHECK(extents("A", &b) == SPSP_OK && b == V({0, 1}));
    CHECK(extents("\n>", &b) == SPSP_OK && b == V({0, 1, 2}));
    CHECK(extents(">a\n>b\n", &b) == SPSP_OK && b == V({0, 3, 6}));
    CHECK(extents("ACGT\nA>C\n>x y\r\nAC\r\n\xffz\nGG", &b) == SPSP_OK && b == V({0, 9, 19, 24}));
    CHECK(keep_all("") == "" && keep_all("A") == "A\n" && keep_all("\n>") == "\n>\n" && keep_all(">a\n>b\n") == ">a\n>b\n");
    uint64_t kept = 0;
    CHECK(extract("ACGT\nA>C\n>x y\r\nAC\r\n\xffz\nGG", {0, 1, 0}, &kept) == ">x y\r\nAC\r\n" && kept == 1);
    CHECK(extract("ACGT\nA>C\n>x y\r\nAC\r\n\xffz\nGG", {0, 0, 1}, &kept) == "\xffz\nGG\n" && kept == 1);
    CHECK(extract("ACGT\nA>C\n>x y\r\nAC\r\n\xffz\nGG", {0, 0, 0}, &kept) == "" && kept == 0);
    CHECK(extract("", {1}, &kept) == "" && kept == 1);

    // FASTQ: quality lines that begin with '@' and '>', the blank tail, the last record without its newline, line counts
    const std::string fq = "@r1\nAC\n+\n@I\n@r2\nG\n+x\n>\n";
    CHECK(extents(fq, &b) == SPSP_OK && b == V({0, 12, 23}));
    CHECK(extents(fq + "\n\r\n\n", &b) == SPSP_OK && b == V({0, 12, 23}));
    CHECK(extents(fq.substr(0, fq.size() - 1), &b) == SPSP_OK && b == V({0, 12, 22}));
    CHECK(extents(fq.substr(0, fq.size() - 1) + "\r\r\n\n", &b) == SPSP_OK && b == V({0, 12, 25}));
    CHECK(extents("@r\nA\n+\n\n", &b) == SPSP_OK && b == V({0, 8}));   // a last, empty read: its quality line is the blank tail's
    CHECK(extents("@r\nA\n+\n\r\n\n", &b) == SPSP_OK && b == V({0, 9}) && extents("@r\nA\n+\n\r", &b) == SPSP_OK && b == V({0, 8}));
    CHECK(extents("@", &b) == SPSP_ERR_FORMAT && extents("@r\nA\n+\n", &b) == SPSP_ERR_FORMAT && extents("@r\nA\n+\nI\n@s", &b) == SPSP_ERR_FORMAT);
    CHECK(extract(fq + "\n\n", {0, 1}, &kept) == "@r2\nG\n+x\n>\n" && kept == 1);
    CHECK(extract(fq.substr(0, fq.size() - 1), {0, 1}, &kept) == "@r2\nG\n+x\n>\n" && kept == 1);
    CHECK(extract(fq.substr(0, fq.size() - 1) + "\r", {1, 1}, &kept) == fq && kept == 2);
    // every prefix of a text: the calls end inside it whatever it is cut at
    const std::string both[2] = {"x\n>a\nAC\n\n>b c\r\nGG\r\n>\n>\n\xff\nT", fq + "\n"};
    for (const std::string& whole : both)
        for (size_t cut = 0; cut <= whole.size(); ++cut) {
            const std::string part = whole.substr(0, cut);
            if (extents(part, &b) != SPSP_OK) continue;
            const std::string all = keep_all(part);
            if (cut == 0 || part[0] != '@') CHECK(all == (part.empty() || part.back() == '\n' ? part : part + "\n"));
        }
    // starts that decrease or leave the text
    {
        Exact t(">a\n>b\n");
        uint64_t* bad = (uint64_t*)malloc(24);
        uint8_t* k = (uint8_t*)malloc(2);
        k[0] = k[1] = 1;
        uint8_t* out = nullptr; uint64_t n_out = 0;
        bad[0] = 0; bad[1] = 4; bad[2] = 3;
        CHECK(spsp_records_extract_host(t.p, t.n, bad, 2, k, &out, &n_out, &kept) == SPSP_ERR_ARG && out == nullptr);
        bad[2] = 7;
        CHECK(spsp_records_extract_host(t.p, t.n, bad, 2, k, &out, &n_out, &kept) == SPSP_ERR_ARG && out == nullptr);
        CHECK(spsp_records_extract_host(t.p, t.n, nullptr, 2, k, &out, &n_out, &kept) == SPSP_ERR_ARG);
        free(bad); free(k);
    }

    // the flag functions: rows in blocks of exactly their sizes
    const uint32_t top = 2, n_ref = 5;
    const uint32_t listed[4] = {0, 1, 2, 2};
    const uint32_t refs[4][2] = {{0, 0}, {3, 0}, {4, 3}, {0, 4}};
    spsp_classify_record* recs = (spsp_classify_record*)calloc(4, sizeof(spsp_classify_record));
    spsp_classify_hit* hits = (spsp_classify_hit*)calloc(4 * top, sizeof(spsp_classify_hit));
    for (int r = 0; r < 4; ++r) {
        recs[r].listed = recs[r].passing = listed[r];
        for (uint32_t i = 0; i < listed[r]; ++i) { hits[r * top + i].reference = refs[r][i]; hits[r * top + i].shared = 9 - i; }
    }
    uint8_t* keep = (uint8_t*)malloc(4);
    auto flags = [&](const char* what) {
        CHECK(spsp_extract_flags_classify_host(what, recs, hits, 4, top, n_ref, keep) == SPSP_OK);
        return std::string(1, (char)('0' + keep[0])) + (char)('0' + keep[1]) + (char)('0' + keep[2]) + (char)('0' + keep[3]);
    };
    CHECK(flags("matched") == "0111" && flags("unmatched") == "1000");
    CHECK(flags("best=3") == "0100" && flags("listed=3") == "0110" && flags("best=4") == "0010" && flags("listed=4") == "0011");
    CHECK(flags("best=0") == "0001" && flags("listed=0") == "0001" && flags("best=1") == "0000" && flags("listed=2") == "0000");
    const char* refused[] = {"", "match", "matchedx", "Matched", "best", "best=", "best=-1", "best= 1", "best=1x", "best=5", "listed=5", "best=4294967296",
                             "listed=99999999999999999999", "classified", "unclassified", "taxon=1", "clade=0", "best=0x1", " matched"};
    for (const char* what : refused) {
        CHECK(spsp_extract_flags_classify_host(what, recs, hits, 4, top, n_ref, keep) == SPSP_ERR_ARG);
        CHECK(strstr(spsp_last_error(), "extract") != nullptr);
    }
    CHECK(spsp_extract_flags_classify_host("matched", recs, hits, 4, 0, n_ref, keep) == SPSP_ERR_ARG);
    CHECK(spsp_extract_flags_classify_host("matched", recs, hits, 4, 1, n_ref, keep) == SPSP_ERR_ARG);   // a record lists two
    CHECK(spsp_extract_flags_classify_host(nullptr, recs, hits, 4, top, n_ref, keep) == SPSP_ERR_ARG);
    CHECK(spsp_extract_flags_classify_host("matched", nullptr, nullptr, 0, top, n_ref, nullptr) == SPSP_OK);

    // tree: 0 root, 1 [1, 4), 2, 3, 4 [4, 6), 5
    const uint32_t T = 6;
    uint32_t* size = (uint32_t*)malloc(T * 4);
    const uint32_t sizes[T] = {6, 3, 1, 1, 2, 1};
    memcpy(size, sizes, sizeof sizes);
    const uint32_t nodes[6] = {SPSP_TAXONOMY_NONE, 0, 1, 3, 4, 5};
    spsp_taxonomy_record* tx = (spsp_taxonomy_record*)calloc(6, sizeof(spsp_taxonomy_record));
    for (int r = 0; r < 6; ++r) tx[r].node = nodes[r];
    uint8_t* keep6 = (uint8_t*)malloc(6);
    auto tflags = [&](const char* what) {
        CHECK(spsp_extract_flags_taxonomy_host(what, tx, 6, size, T, keep6) == SPSP_OK);
        std::string s;
        for (int r = 0; r < 6; ++r) s += (char)('0' + keep6[r]);
        return s;
    };
    CHECK(tflags("classified") == "011111" && tflags("unclassified") == "100000");
    CHECK(tflags("taxon=0") == "010000" && tflags("taxon=1") == "001000" && tflags("taxon=2") == "000000" && tflags("taxon=5") == "000001");
    CHECK(tflags("clade=0") == "011111" && tflags("clade=1") == "001100" && tflags("clade=4") == "000011" && tflags("clade=3") == "000100" && tflags("clade=2") == "000000");
    const char* trefused[] = {"", "classifie", "taxon", "taxon=", "clade=6", "taxon=6", "clade=x", "matched", "unmatched", "best=0", "listed=1", "clade=1 "};
    for (const char* what : trefused) {
        CHECK(spsp_extract_flags_taxonomy_host(what, tx, 6, size, T, keep6) == SPSP_ERR_ARG);
        CHECK(strstr(spsp_last_error(), "extract") != nullptr);
    }
    CHECK(spsp_extract_flags_taxonomy_host("classified", tx, 6, size, 0, keep6) == SPSP_ERR_ARG);
    CHECK(spsp_extract_flags_taxonomy_host("classified", tx, 6, nullptr, T, keep6) == SPSP_ERR_ARG);
    // every word cut off at every length, in a block of exactly its size (and its 0 byte)
    const char* words[] = {"matched", "unmatched", "best=12", "listed=3", "classified", "unclassified", "taxon=41", "clade=5"};
    for (const char* w : words)
        for (size_t cut = 0; cut <= strlen(w); ++cut) {
            char* part = (char*)malloc(cut + 1);
            memcpy(part, w, cut);
            part[cut] = 0;
            const int a = spsp_extract_word_check_host(part, 0, 0xffffffffu), c = spsp_extract_word_check_host(part, 1, 0xffffffffu);
            CHECK((a == SPSP_OK || a == SPSP_ERR_ARG) && (c == SPSP_OK || c == SPSP_ERR_ARG) && !(a == SPSP_OK && c == SPSP_OK));
            if (cut == strlen(w)) CHECK(a == SPSP_OK || c == SPSP_OK);
            free(part);
        }
    CHECK(spsp_extract_word_check_host("best=1", 0, 1) == SPSP_ERR_ARG && spsp_extract_word_check_host("best=0", 0, 1) == SPSP_OK);
    CHECK(spsp_extract_word_check_host(nullptr, 0, 1) == SPSP_ERR_ARG);
    free(recs); free(hits); free(keep); free(size); free(tx); free(keep6);
    printf("extract_asan: ok\n");
    return 0;
}
