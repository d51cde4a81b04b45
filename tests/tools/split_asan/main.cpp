// The host half of the split -- the rule as plain loops (spsp_records_split_host), the two bin functions with their refusals
// (spsp_split_bins_classify_host, spsp_split_bins_taxonomy_host, spsp_split_word_check_host), the manifest's text
// (spsp_split_csv_host) and the plan -- driven on the CPU by a program of its own, so that it can be built with AddressSanitizer +
// UBSan (run.sh).  No device, no Python.  Every buffer handed in has its exact size on the heap and no 0 byte behind a text: a read
// behind text[n - 1], bin[n_rec - 1], hits[n * top - 1], parent[T - 1] or depth[T - 1] is ASan's to find.
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

// a copy of `v` in a heap block of exactly its size
template <class T> struct Exact {
    T* p;
    size_t n;
    explicit Exact(const std::vector<T>& v) : p((T*)malloc(v.size() ? v.size() * sizeof(T) : 1)), n(v.size()) { if (n) memcpy(p, v.data(), n * sizeof(T)); }
    ~Exact() { free(p); }
};
static std::vector<uint8_t> bytes_of(const std::string& s) { return std::vector<uint8_t>(s.begin(), s.end()); }
static bool said(const char* word) { return strstr(spsp_last_error(), word) != nullptr; }

struct Split { int rc; std::string out; std::vector<uint64_t> off, records; };

static Split split(const std::string& text, const std::vector<uint32_t>& bin, uint32_t n_bins, const std::vector<uint64_t>* own_begin = nullptr) {
    Exact<uint8_t> t(bytes_of(text));
    std::vector<uint64_t> begin;
    if (own_begin) begin = *own_begin;
    else {
        uint64_t* b = nullptr; uint32_t n_rec = 0;
        CHECK(spsp_records_extents_host(t.n ? t.p : nullptr, t.n, &b, &n_rec) == SPSP_OK && n_rec == bin.size());
        begin.assign(b, b + n_rec + 1);
        spsp_free(b);
    }
    Exact<uint64_t> b(begin);
    Exact<uint32_t> k(bin);
    Split s;
    uint8_t* out = nullptr; uint64_t n_out = 0, *off = nullptr, *rec = nullptr;
    s.rc = spsp_records_split_host(t.n ? t.p : nullptr, t.n, b.p, (uint32_t)bin.size(), k.p, n_bins, &out, &n_out, &off, &rec);
    if (s.rc == SPSP_OK) {
        s.out.assign((const char*)out, (size_t)n_out);
        s.off.assign(off, off + n_bins + 1);
        s.records.assign(rec, rec + n_bins);
        spsp_free(out); spsp_free(off); spsp_free(rec);
    } else CHECK(out == nullptr && off == nullptr && rec == nullptr && n_out == 0);
    return s;
}

int main() {
    const uint32_t DROP = SPSP_SPLIT_DROP;
    uint32_t stretch = 0, rec_tile = 0, sort_tile = 0, max_bins = 0;
    CHECK(spsp_split_plan_host(&stretch, &rec_tile, &sort_tile, &max_bins) == SPSP_OK && stretch == 16384 && rec_tile == 2048 && sort_tile == 2048 &&
          max_bins == SPSP_SPLIT_MAX_BINS);
    CHECK(spsp_split_plan_host(nullptr, nullptr, nullptr, nullptr) == SPSP_OK);

    // the rule: three bins, a DROP, empty bins, the last record without its newline in bin 0
    const std::string fa = ">a\nAC\n>b\nGG\n>c\nT\n>d\nCC";
    Split s = split(fa, {2, 0, DROP, 0}, 3);
    CHECK(s.rc == SPSP_OK && s.out == ">b\nGG\n>d\nCC\n>a\nAC\n" && s.off == (std::vector<uint64_t>{0, 12, 12, 18}) && s.records == (std::vector<uint64_t>{2, 0, 1}));
    s = split(fa, {1, 1, 1, 1}, 4);
    CHECK(s.rc == SPSP_OK && s.out == fa + "\n" && s.off == (std::vector<uint64_t>{0, 0, 23, 23, 23}));
    s = split(fa, {DROP, DROP, DROP, DROP}, 1);
    CHECK(s.rc == SPSP_OK && s.out.empty() && s.off == (std::vector<uint64_t>{0, 0}) && s.records == (std::vector<uint64_t>{0}));
    s = split("", {0}, 2);                                   // the empty text: one empty record, which counts and adds nothing
    CHECK(s.rc == SPSP_OK && s.out.empty() && s.records == (std::vector<uint64_t>{1, 0}));
    const std::string fq = "@r1\nACGT\n+\nIIII\n@r2\nAC\n+\nII";
    s = split(fq, {1, 0}, 2);
    CHECK(s.rc == SPSP_OK && s.out == "@r2\nAC\n+\nII\n@r1\nACGT\n+\nIIII\n" && s.off == (std::vector<uint64_t>{0, 12, 28}));
    const std::vector<uint64_t> own = {0, 3, 3, 7, 9};       // ranges of the caller's, one of them empty; only the last is looked at for the newline
    s = split("abcdefghi", {1, 1, 0, 1}, 2, &own);
    CHECK(s.rc == SPSP_OK && s.out == "defgabchi\n" && s.records == (std::vector<uint64_t>{1, 3}) && s.off == (std::vector<uint64_t>{0, 4, 10}));
    // refusals
    s = split(fa, {0, 1, 3, 0}, 3);
    CHECK(s.rc == SPSP_ERR_ARG && said("bin[2] = 3"));
    s = split(fa, {0, 0, 0, 0}, 0);
    CHECK(s.rc == SPSP_ERR_ARG && said("n_bins = 0"));
    s = split(fa, {0, 0, 0, 0}, SPSP_SPLIT_MAX_BINS + 1);
    CHECK(s.rc == SPSP_ERR_ARG && said("n_bins = 16777217"));
    const std::vector<uint64_t> bad1 = {0, 5, 4}, bad2 = {0, 4, 10};
    CHECK(split("abcdefghi", {0, 0}, 1, &bad1).rc == SPSP_ERR_ARG && said("begin"));
    CHECK(split("abcdefghi", {0, 0}, 1, &bad2).rc == SPSP_ERR_ARG && said("begin"));

    // the bins of classify's rows
    {
        const uint32_t top = 2, n_ref = 5;
        std::vector<spsp_classify_record> recs(4, spsp_classify_record{});
        std::vector<spsp_classify_hit> hits(4 * top, spsp_classify_hit{});
        recs[1].listed = 1; hits[1 * top] = {3, 9};
        recs[2].listed = 2; hits[2 * top] = {4, 9}; hits[2 * top + 1] = {0, 8};
        recs[3].listed = 1; hits[3 * top] = {0, 2};
        Exact<spsp_classify_record> r(recs);
        Exact<spsp_classify_hit> h(hits);
        Exact<uint32_t> bin(std::vector<uint32_t>(4, 77));
        uint32_t n_bins = 0;
        CHECK(spsp_split_bins_classify_host("best", r.p, h.p, 4, top, n_ref, bin.p, &n_bins) == SPSP_OK && n_bins == 6);
        CHECK(bin.p[0] == 5 && bin.p[1] == 3 && bin.p[2] == 4 && bin.p[3] == 0);
        for (const char* what : {"", "Best", "best=1", "bestx", "matched", "depth", "depth=", "depth=1x"}) {
            CHECK(spsp_split_bins_classify_host(what, r.p, h.p, 4, top, n_ref, bin.p, &n_bins) == SPSP_ERR_ARG && said("names no bins") && n_bins == 0);
            CHECK(spsp_split_word_check_host(what, 0) == SPSP_ERR_ARG && spsp_split_word_check_host(what, 1) == SPSP_ERR_ARG);
        }
        for (const char* what : {"taxon", "depth=2"})
            CHECK(spsp_split_bins_classify_host(what, r.p, h.p, 4, top, n_ref, bin.p, &n_bins) == SPSP_ERR_ARG && said("taxonomy's rows") && said(what));
        CHECK(spsp_split_bins_classify_host("best", r.p, h.p, 4, top, 4, bin.p, &n_bins) == SPSP_ERR_ARG && said("record 2"));   // a reference the index does not have
        r.p[3].listed = 3;
        CHECK(spsp_split_bins_classify_host("best", r.p, h.p, 4, top, n_ref, bin.p, &n_bins) == SPSP_ERR_ARG && said("top = 2"));
        CHECK(spsp_split_bins_classify_host("best", nullptr, nullptr, 0, top, n_ref, nullptr, &n_bins) == SPSP_OK && n_bins == 6);
    }
    // the bins of a taxonomy's rows.  0 root; 1 (depth 1); 2 (2); 3 (3); 4 (3); 5 (1); 6 (2)
    {
        const std::vector<uint32_t> parent = {0, 0, 1, 2, 2, 0, 5}, depth = {0, 1, 2, 3, 3, 1, 2};
        Exact<uint32_t> p(parent), d(depth);
        std::vector<spsp_taxonomy_record> recs(8, spsp_taxonomy_record{});
        const uint32_t node[8] = {SPSP_TAXONOMY_NONE, 0, 1, 2, 3, 4, 5, 6};
        for (int i = 0; i < 8; ++i) recs[i].node = node[i];
        Exact<spsp_taxonomy_record> r(recs);
        Exact<uint32_t> bin(std::vector<uint32_t>(8, 77));
        uint32_t n_bins = 0;
        const auto expect = [&](const char* what, std::vector<uint32_t> want) {
            CHECK(spsp_split_bins_taxonomy_host(what, r.p, 8, p.p, d.p, 7, bin.p, &n_bins) == SPSP_OK && n_bins == 8);
            for (int i = 0; i < 8; ++i) CHECK(bin.p[i] == want[i]);
        };
        expect("taxon", {7, 0, 1, 2, 3, 4, 5, 6});
        expect("depth=1", {7, 0, 1, 1, 1, 1, 5, 5});
        expect("depth=2", {7, 0, 1, 2, 2, 2, 5, 6});
        expect("depth=3", {7, 0, 1, 2, 3, 4, 5, 6});
        expect("depth=32", {7, 0, 1, 2, 3, 4, 5, 6});
        for (const char* what : {"depth=0", "depth=33", "depth=4294967295"})
            CHECK(spsp_split_bins_taxonomy_host(what, r.p, 8, p.p, d.p, 7, bin.p, &n_bins) == SPSP_ERR_ARG && said(what) && said("1 .. 32") &&
                  spsp_split_word_check_host(what, 1) == SPSP_ERR_ARG);
        CHECK(spsp_split_bins_taxonomy_host("best", r.p, 8, p.p, d.p, 7, bin.p, &n_bins) == SPSP_ERR_ARG && said("classify's rows"));
        CHECK(spsp_split_word_check_host("best", 0) == SPSP_OK && spsp_split_word_check_host("taxon", 1) == SPSP_OK && spsp_split_word_check_host("depth=7", 1) == SPSP_OK);
        r.p[4].node = 7;
        CHECK(spsp_split_bins_taxonomy_host("taxon", r.p, 8, p.p, d.p, 7, bin.p, &n_bins) == SPSP_ERR_ARG && said("record 4"));
    }
    // the manifest
    {
        const char* names[3] = {"refA", "refB", "refC"};
        const std::vector<uint64_t> records = {2, 0, 1, 4}, off = {0, 10, 10, 15, 40}, off2 = {0, 12, 12, 18, 50};
        Exact<uint64_t> r(records), o(off), o2(off2);
        char* text = nullptr; uint64_t len = 0;
        CHECK(spsp_split_csv_host("run", names, "unmatched", 4, r.p, o.p, ".fq.gz", nullptr, nullptr, &text, &len) == SPSP_OK);
        CHECK(std::string(text, len) == "bin,name,records,bytes,file\n0,refA,2,10,run_split_0.fq.gz\n2,refC,1,5,run_split_2.fq.gz\n"
                                        "unmatched,unmatched,4,25,run_split_unmatched.fq.gz\n");
        spsp_free(text);
        CHECK(spsp_split_csv_host("run", names, "unmatched", 4, r.p, o.p, ".fq", o2.p, ".fa", &text, &len) == SPSP_OK);
        CHECK(std::string(text, len) == "bin,name,records,bytes_1,file_1,bytes_2,file_2\n0,refA,2,10,run_split_0_1.fq,12,run_split_0_2.fa\n"
                                        "2,refC,1,5,run_split_2_1.fq,6,run_split_2_2.fa\nunmatched,unmatched,4,25,run_split_unmatched_1.fq,32,run_split_unmatched_2.fa\n");
        spsp_free(text);
        CHECK(spsp_split_csv_host("run", names, "unmatched", 0, r.p, o.p, ".fq", nullptr, nullptr, &text, &len) == SPSP_ERR_ARG && text == nullptr);
    }
    printf("split_asan: ok\n");
    return 0;
}
