// The host half of "raw coordinates" -- the lift as plain loops (spsp_records_lift_host), the BED text (spsp_segments_bed_host) and
// the plan -- driven on the CPU by a program of its own, so that it can be built with AddressSanitizer + UBSan (run.sh).  No
// device, no Python.  Every buffer handed in has its exact size on the heap: a read behind text[n - 1] or h_base[n_q - 1], or a
// write behind raw[n_q - 1], rec[n_q - 1] or raw_length[n_rec - 1], is ASan's to find.
#include <algorithm>
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

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, spsp_last_error()); exit(1); } \
    } while (0)

// a copy of `v` in a heap block of exactly its size
template <class T> struct Exact {
    T* p;
    size_t n;
    explicit Exact(const std::vector<T>& v) : p((T*)malloc(v.size() ? v.size() * sizeof(T) : 1)), n(v.size()) { if (n) memcpy(p, v.data(), n * sizeof(T)); }
    explicit Exact(size_t count) : p((T*)malloc(count ? count * sizeof(T) : 1)), n(count) {}
    ~Exact() { free(p); }
};
static bool said(const char* word) { return strstr(spsp_last_error(), word) != nullptr; }

// the rule once more, byte by byte with nothing shared: per kept base its record and its raw position; per record its length
struct Lifted { std::vector<uint64_t> raw; std::vector<uint32_t> rec; std::vector<uint64_t> len; };
static Lifted model(const std::string& t) {
    Lifted m;
    const bool fastq = !t.empty() && t[0] == '@';
    m.len.push_back(0);
    uint64_t line = 0;
    bool line_start = true, data = false;
    for (size_t i = 0; i < t.size(); ++i) {
        const unsigned char c = (unsigned char)t[i];
        if (line_start) {
            if (fastq) {
                if (line % 4 == 0 && line > 0 && c != '\n' && c != '\r') m.len.push_back(0);
                data = line % 4 == 1;
            } else {
                const bool begins = line == 0 || c == '>' || c == 0xFF;
                if (begins && line > 0) m.len.push_back(0);
                data = !begins;
            }
            line_start = false;
        }
        if (c == '\n') { ++line; line_start = true; continue; }
        if (!data || c < 0x21 || c > 0x7e) continue;
        if (strchr("ACGTacgt", c)) { m.raw.push_back(m.len.back()); m.rec.push_back((uint32_t)(m.len.size() - 1)); }
        ++m.len.back();
    }
    return m;
}

// every kept base, then a sorted sample with repeats, against the model; raw_length with its exact room
static void lift_case(const std::string& t, std::mt19937_64& rng) {
    const Lifted m = model(t);
    const Exact<uint8_t> text(std::vector<uint8_t>(t.begin(), t.end()));
    uint32_t n_rec = 0;
    CHECK(spsp_records_lift_host(text.p, text.n, nullptr, 0, nullptr, nullptr, nullptr, &n_rec) == SPSP_OK && n_rec == m.len.size());
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<uint64_t> base;
        if (pass == 0) for (uint64_t g = 0; g < m.raw.size(); ++g) base.push_back(g);
        else if (!m.raw.empty()) {
            for (int i = 0; i < 40; ++i) base.push_back(rng() % m.raw.size());
            std::sort(base.begin(), base.end());
        }
        const Exact<uint64_t> b(base);
        Exact<uint64_t> raw(base.size()), len(m.len.size());
        Exact<uint32_t> rec(base.size());
        n_rec = (uint32_t)m.len.size();
        CHECK(spsp_records_lift_host(text.p, text.n, b.p, b.n, raw.p, rec.p, len.p, &n_rec) == SPSP_OK && n_rec == m.len.size());
        for (size_t q = 0; q < base.size(); ++q) CHECK(raw.p[q] == m.raw[base[q]] && rec.p[q] == m.rec[base[q]]);
        for (size_t r = 0; r < m.len.size(); ++r) CHECK(len.p[r] == m.len[r]);
        CHECK(spsp_records_lift_host(text.p, text.n, b.p, b.n, raw.p, nullptr, nullptr, &n_rec) == SPSP_OK);   // rec and raw_length may be NULL
    }
    // refusals: an index that is not below the kept bases; indices that decrease; a raw_length of the wrong room
    {
        const Exact<uint64_t> b(std::vector<uint64_t>{(uint64_t)m.raw.size()});
        Exact<uint64_t> raw(1);
        CHECK(spsp_records_lift_host(text.p, text.n, b.p, 1, raw.p, nullptr, nullptr, &n_rec) == SPSP_ERR_ARG && said("not below"));
        Exact<uint64_t> len(m.len.size() + 1);
        n_rec = (uint32_t)m.len.size() + 1;
        CHECK(spsp_records_lift_host(text.p, text.n, nullptr, 0, nullptr, nullptr, len.p, &n_rec) == SPSP_ERR_ARG && said("room"));
    }
    if (m.raw.size() >= 2) {
        const Exact<uint64_t> b(std::vector<uint64_t>{1, 0});
        Exact<uint64_t> raw(2);
        CHECK(spsp_records_lift_host(text.p, text.n, b.p, 2, raw.p, nullptr, nullptr, &n_rec) == SPSP_ERR_ARG && said("decrease"));
    }
}

static std::string random_text(std::mt19937_64& rng, bool fastq, size_t n_rec) {
    const char* soup = "ACGTACGTacgtNnRY-* \t";
    const auto run = [&](size_t n) { std::string s; for (size_t i = 0; i < n; ++i) s += soup[rng() % 20]; return s; };
    std::string t;
    for (size_t r = 0; r < n_rec; ++r) {
        if (fastq) {
            const size_t L = rng() % 90;
            t += "@r" + std::to_string(r) + " ACGT\n" + run(L) + (rng() % 5 ? "\n" : "\r\n") + "+\n" + (rng() % 2 ? ">@ACGT" : "") + run(L) + "\n";
        } else {
            t += (rng() % 7 ? ">" : "\xff") + std::string("r") + std::to_string(r) + " ACGT\n";
            for (size_t lines = rng() % 4; lines; --lines) t += run(rng() % 70) + (rng() % 5 ? "\n" : "\r\n");
        }
    }
    if (!t.empty() && rng() % 2) t.pop_back();             // a text without its last newline
    if (fastq && rng() % 3 == 0) t += "\n\n\r\n";          // the blank tail
    return t;
}

int main() {
    std::mt19937_64 rng(20260117);
    uint32_t tile = 0, chunk = 0;
    CHECK(spsp_lift_plan_host(&tile, &chunk) == SPSP_OK && tile == 4096 && chunk == 16 && spsp_lift_plan_host(nullptr, nullptr) == SPSP_OK);
    for (const char* t : {"", "\n", "ACGT", "ACGT\nACNGT\n>r1\n\n>r2\nNNNN\n>r3\nAC GT\tA\r\nac-gt", ">a\n\xff" "b\nACGT\n", ">only a header", "@r\nACNGT\n+\n>@ACG\n",
                          "@r\nAC\n+\nII\n@s\n\n+\n\n\n\n", "@", "@r\nACGT"})
        lift_case(t, rng);
    for (int i = 0; i < 60; ++i) lift_case(random_text(rng, i % 2 == 1, 1 + rng() % 12), rng);

    // the BED text: the empty segment is left out, the tab in a call's name becomes a blank
    std::vector<spsp_segment_row> segs(3);
    segs[0] = spsp_segment_row{0, 10, 5, 4, 3, 0, 0, 2, 0};
    segs[1] = spsp_segment_row{0, 0, 0, 0, 0, 1, 0, 1, 2};
    segs[2] = spsp_segment_row{10, 30, 9, 0, 0, 2, 1, 4, 1};
    const Exact<spsp_segment_row> s(segs);
    const Exact<uint64_t> rb(std::vector<uint64_t>{3, 0, 17}), re(std::vector<uint64_t>{15, 0, 40});
    const char* names[] = {"chr1", "empty", "chr2"};
    const char* calls[] = {"ref A", "ref\tB"};
    char* text = nullptr; uint64_t len = 0;
    CHECK(spsp_segments_bed_host(s.p, 3, rb.p, re.p, names, 3, calls, "unmatched", 3, &text, &len) == SPSP_OK);
    const std::string want = "chr1\t3\t15\tref A\t0\t.\t0\t0\t10\t2\t3\nchr2\t17\t40\tref B\t0\t.\t1\t10\t30\t4\t0\n";
    CHECK(len == want.size() && std::string(text, len) == want);
    spsp_free(text);
    const Exact<uint64_t> short_end(std::vector<uint64_t>{12, 0, 40});
    CHECK(spsp_segments_bed_host(s.p, 3, rb.p, short_end.p, names, 3, calls, "unmatched", 3, &text, &len) == SPSP_ERR_ARG && said("shorter") && !text);
    CHECK(spsp_segments_bed_host(s.p, 3, rb.p, re.p, names, 2, calls, "unmatched", 3, &text, &len) == SPSP_ERR_ARG && said("out of range"));
    CHECK(spsp_segments_bed_host(s.p, 3, rb.p, re.p, names, 3, calls, "unmatched", 2, &text, &len) == SPSP_ERR_ARG);
    CHECK(spsp_segments_bed_host(nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, "unmatched", 1, &text, &len) == SPSP_OK && len == 0);
    spsp_free(text);
    printf("lift_asan: ok\n");
    return 0;
}
