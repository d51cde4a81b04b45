// comparator -- drop-in command line of the reference's comparator
// (Comparator.cpp:464-521) over libspsp: same flags, defaults, messages and
// output files (<o>_containment.csv.gz, <o>_jaccard.csv.gz).  One addition: -g <min_keys> with -q gathers instead --
// which references make up each query, greedily (spsp_gather_files) -> <o>_gather.csv.gz.  Another: -c <t> / -C <t> without -q
// clusters the index instead -- single linkage on Jaccard / on the larger containment at threshold t (spsp_cluster_files) ->
// <o>_clusters.csv.gz.  A third: -N <top> [-J <t> | -K <t> | -I <t>], with or without -q, lists each sketch's (each query's) best
// <top> partners at or above threshold t instead -- on Jaccard, on the larger containment, on the row's containment in the
// partner; Jaccard at 0 with none of the three (spsp_neighbours_files) -> <o>_neighbours.csv.gz.  A fourth: -P <t>, with or
// without -q, counts instead how many of the index's sketches hold each key -- per sketch (per query) the keys that are core (held
// by a share t of the index or more), shell, unique and absent, and the spectrum of the index's union (spsp_prevalence_files) ->
// <o>_prevalence.csv.gz and <o>_spectrum.csv.gz.  A fifth: -r <t> / -R <t> without -q picks representatives of the index instead --
// greedy dereplication on Jaccard / on the larger containment at threshold t, best sketch first: by the weights of -w <file> (one
// unsigned integer per sketch of -f, in list order), else by key count (spsp_representatives_files) -> <o>_representatives.csv.gz.
// A sixth: -l <floor> / -L <floor> without -q builds the index's single-linkage tree instead -- on Jaccard / on the larger containment,
// over the pairs at or above the floor, 0 for every pair that shares a key (spsp_tree_files) -> <o>_tree.csv.gz and <o>_tree.nwk.
// A seventh: -S <what> without -q / -E <what> with or without -q writes SKETCHES instead -- the keys whose number of holders in the
// index lies in the band <what> names (union, present, absent, all, core=<t>, unique=<t>, shell=<t>, <a>..<b>): -S the distinct
// keys of the index as one sketch, <o>_select.gz; -E every sketch's (every query's) own, <o>_<i>_<its file name>, listed in
// <o>_select.txt (spsp_select_files).  An eighth: -A <orders> [-z <seed>] without -q draws the index's accumulation curves instead -- the
// size of the union (pan) and of the intersection (core) of the first j sketches, over <orders> orders of them: the list order and
// shuffles drawn from the seed, 1 unless -z names it (spsp_accumulation_files) -> <o>_accumulation.csv.gz.  A ninth: -G <labels file>
// [-T <t>] [-U <u>] [-M] without -q reads one group label per sketch of -f and counts, per group, the keys its members hold, share
// (at least <t> of them, default 1), hold alone, and are identified by (shared, and held by at most <u> of the others, default 0)
// (spsp_groups_files) -> <o>_groups.csv.gz, <o>_members.csv.gz and, with -M, one marker sketch per group listed in <o>_markers.txt.
#include <getopt.h>

#include <chrono>
#include <iostream>
#include <sstream>
#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/spsp.h"

using namespace std;

// Comparator::getfilesname (Comparator.cpp:7-21): lines longer than 2 chars
static bool read_names(const string& fof, vector<string>& out) {
    uint8_t* data = nullptr; uint64_t len = 0;
    if (spsp_read_file_host(fof.c_str(), &data, &len) != SPSP_OK) { cout << "Can't open " << fof << endl; return false; }
    istringstream is(string((const char*)data, len));
    spsp_free(data);
    string line;
    while (getline(is, line))
        if (line.size() > 2) out.push_back(line);
    return true;
}

// -c / -C <t>: a decimal in (0, 1] with at most six digits behind the point, read as TEXT into num / 10^digits ("0.95" = 95 / 100,
// "1" = 1 / 1): the threshold takes part in integer comparisons only.  -J / -K / -I <t> admit 0 as well (zero_ok)
static bool parse_fraction(const char* t, uint32_t* num, uint32_t* den, bool zero_ok = false) {
    if ((t[0] != '0' && t[0] != '1') || (t[1] != 0 && t[1] != '.')) return false;
    uint64_t n = (uint64_t)(t[0] - '0'), d = 1;
    if (t[1] == '.') {
        const char* f = t + 2;
        if (*f == 0) return false;
        for (; *f; ++f) {
            if (*f < '0' || *f > '9' || d >= 1000000) return false;
            n = n * 10 + (uint64_t)(*f - '0'); d *= 10;
        }
    }
    if ((n < 1 && !zero_ok) || n > d) return false;
    *num = (uint32_t)n; *den = (uint32_t)d;
    return true;
}

// -w <file>: one unsigned decimal integer below 2^47 per sketch, in list order (blank lines are skipped)
static bool read_weights(const string& path, size_t n, vector<uint64_t>& out, string& why) {
    uint8_t* data = nullptr; uint64_t len = 0;
    if (spsp_read_file_host(path.c_str(), &data, &len) != SPSP_OK) { why = "can't open it"; return false; }
    istringstream is(string((const char*)data, len));
    spsp_free(data);
    string line;
    while (getline(is, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty()) continue;
        uint64_t v = 0;
        for (char c : line) {
            if (c < '0' || c > '9') { why = "'" + line + "' is not an unsigned integer"; return false; }
            v = v * 10 + (uint64_t)(c - '0');
            if (v >> 47) { why = "'" + line + "' is not below 2^47"; return false; }
        }
        out.push_back(v);
    }
    if (out.size() != n) { why = to_string(out.size()) + " weights for " + to_string(n) + " sketches"; return false; }
    return true;
}

int main(int argc, char** argv) {
    int ch;
    string inputfof, query, output_name("results");
    uint64_t p = 6;
    double min_threshold = 0;
    double rate = SPSP_RATE_AS_IS;   // -s <rate> / -s auto: compare at a common sampling rate (not in the reference, which parses and ignores -s)
    bool gather = false;             // -g <min_keys>: the reference parses -g and ignores it
    uint64_t min_keys = 0;
    int cluster_opts = 0, cluster_metric = SPSP_CLUSTER_JACCARD;   // -c <t> / -C <t>: neither letter is in the reference's option string
    uint32_t cluster_num = 0, cluster_den = 1;
    // -N <top> and -J / -K / -I <t>: none of the four letters is in the reference's option string
    bool neighbours = false;
    long long top = 0;
    int nb_opts = 0, nb_metric = SPSP_NEIGHBOUR_JACCARD;
    uint32_t nb_num = 0, nb_den = 1;
    bool prevalence = false;         // -P <t>: the letter is not in the reference's option string
    uint32_t pv_num = 0, pv_den = 1;
    int rep_opts = 0, rep_metric = SPSP_CLUSTER_JACCARD;   // -r <t> / -R <t>, -w <file>: none of the three letters is in the reference's option string
    uint32_t rep_num = 0, rep_den = 1;
    string weights_file;
    int tree_opts = 0, tree_metric = SPSP_CLUSTER_JACCARD;   // -l <floor> / -L <floor>: neither letter is in the reference's option string
    uint32_t tree_num = 0, tree_den = 1;
    int select_opts = 0;             // -S <what> / -E <what>: neither letter is in the reference's option string
    bool select_each = false;
    string select_what;
    long long acc_orders = 0;        // -A <orders> [-z <seed>]: neither letter is in the reference's option string
    bool accumulation = false, acc_seeded = false;
    uint64_t acc_seed = 1;
    string labels_file;              // -G <labels file> [-T <t>] [-U <u>] [-M]: none of the four letters is in the reference's option string
    bool groups = false, gp_markers = false;
    int gp_opts = 0;                 // -T, -U or -M seen
    uint32_t gp_num = 1, gp_den = 1, gp_onum = 0, gp_oden = 1;
    string records_file;             // -X <records file> [-Y <top>] [-V <min_keys>] [-I <t>]: -X, -Y and -V are not in the reference's option string
    bool classify = false;
    string mates_file;               // -x <mates file>: with -X, record p of the two files is one pair (not in the reference's option string)
    bool paired = false;
    int cf_opts = 0;                 // -Y or -V seen
    long long cf_top = 1, cf_min_keys = 1;
    string lineages_file;            // -H <lineages file>: with -X, the records go to the lowest common ancestor of their keys (not in the reference's option string)
    bool taxonomy = false, cf_top_seen = false;
    string extract_what;             // -F <what> [-u]: with -X, the records the word names are written out again (neither letter is in the reference's option string)
    bool extract = false, extract_plain = false;
    string split_what;               // -j <word> [-u]: with -X, every record goes to the file of its reference or taxon (not in the reference's option string)
    bool split = false;
    string window_arg;               // -y <W>[:<word>]: with -X, every record is cut into windows of W bases and called stretch by stretch (not in the reference's option string)
    bool windows = false;
    long long smooth_q = 0;          // -Q <q>: with -y, stray runs of up to q windows take their neighbours' call (not in the reference's option string)
    bool smooth = false;
    string segments_arg;             // -Z <what>[:<min_bases>]: with -y, the segments the word names are written as <prefix>_segments.fa.gz (likewise)
    bool segments = false;
    bool raw_coords = false;         // -O: with -y, the segments in the records file's own coordinates as <prefix>_segments.bed.gz (-u: plain)
    vector<string> reads_files;      // -D <reads file> [-D <more> ...] [-W <min_count>]: neither letter is in the reference's option string
    bool dp_min_seen = false;
    long long dp_min_count = 1;
    bool profile = false;            // -B <min_keys>: the profile behind the depth of -D (not in the reference's option string either)
    long long pf_min_keys = 1;
    while ((ch = getopt(argc, argv, "hdag:q:k:m:n:s:t:b:e:f:i:p:o:c:C:N:J:K:I:P:r:R:w:l:L:S:E:A:z:G:T:U:MX:Y:V:D:W:B:H:F:ux:j:y:Q:Z:O")) != -1) {
        switch (ch) {
            case 'D': reads_files.push_back(optarg); break;
            case 'W': {
                char* e = nullptr;
                dp_min_count = strtoll(optarg, &e, 10);
                if (e == optarg || *e || dp_min_count < 1 || dp_min_count > 0xffffffffll) { cout << "-W takes the smallest number of records a found key is held by, an integer in 1 .. 4294967295, not '" << optarg << "'" << endl; return 1; }
                dp_min_seen = true;
                break;
            }
            case 'B': {
                char* e = nullptr;
                pf_min_keys = strtoll(optarg, &e, 10);
                if (e == optarg || *e || pf_min_keys < 1 || pf_min_keys > 0xffffffffll) { cout << "-B takes the smallest number of live keys a named reference has, an integer in 1 .. 4294967295, not '" << optarg << "'" << endl; return 1; }
                profile = true;
                break;
            }
            case 'G': labels_file = optarg; groups = true; break;
            case 'X': records_file = optarg; classify = true; break;
            case 'x': mates_file = optarg; paired = true; break;
            case 'H': lineages_file = optarg; taxonomy = true; break;
            case 'F': extract_what = optarg; extract = true; break;
            case 'u': extract_plain = true; break;
            case 'j': split_what = optarg; split = true; break;
            case 'y': window_arg = optarg; windows = true; break;
            case 'Q': {
                char* e = nullptr;
                smooth_q = strtoll(optarg, &e, 10);
                if (e == optarg || *e || optarg[0] == '+' || smooth_q < 0 || smooth_q > 0x7fffffffll) { cout << "-Q takes the longest stray run that is absorbed, in windows, an integer in 0 .. 2147483647, not '" << optarg << "'" << endl; return 1; }
                smooth = true;
                break;
            }
            case 'Z': segments_arg = optarg; segments = true; break;
            case 'O': raw_coords = true; break;
            case 'Y': {
                char* e = nullptr;
                cf_top = strtoll(optarg, &e, 10);
                if (e == optarg || *e || cf_top < 1 || cf_top > 64) { cout << "-Y takes the number of matches listed per record, an integer in 1 .. 64, not '" << optarg << "'" << endl; return 1; }
                ++cf_opts;
                cf_top_seen = true;
                break;
            }
            case 'V': {
                char* e = nullptr;
                cf_min_keys = strtoll(optarg, &e, 10);
                if (e == optarg || *e || cf_min_keys < 1 || cf_min_keys > 0xffffffffll) { cout << "-V takes the smallest number of shared keys a match is listed for, an integer >= 1, not '" << optarg << "'" << endl; return 1; }
                ++cf_opts;
                break;
            }
            case 'T':
                if (!parse_fraction(optarg, &gp_num, &gp_den)) {
                    cout << "-T takes the share of a group's members that makes a key core, in (0, 1] with at most six digits behind the point, not '" << optarg << "'" << endl;
                    return 1;
                }
                ++gp_opts;
                break;
            case 'U':
                if (!parse_fraction(optarg, &gp_onum, &gp_oden, true)) {
                    cout << "-U takes the share of the other sketches that may hold a marker, in [0, 1] with at most six digits behind the point, not '" << optarg << "'" << endl;
                    return 1;
                }
                ++gp_opts;
                break;
            case 'M': gp_markers = true; ++gp_opts; break;
            case 'A': {
                char* e = nullptr;
                acc_orders = strtoll(optarg, &e, 10);
                if (e == optarg || *e || acc_orders < 1 || acc_orders > 1024) { cout << "-A takes the number of orders the curves are taken over, an integer in 1 .. 1024, not '" << optarg << "'" << endl; return 1; }
                accumulation = true;
                break;
            }
            case 'z': {
                char* e = nullptr;
                errno = 0;
                acc_seed = strtoull(optarg, &e, 10);
                if (e == optarg || *e || errno || optarg[0] == '-') { cout << "-z takes the seed of the orders, an unsigned 64-bit integer, not '" << optarg << "'" << endl; return 1; }
                acc_seeded = true;
                break;
            }
            case 'S':
            case 'E': {
                uint32_t a = 0, b = 0;
                if (spsp_select_band_host(optarg, 1, &a, &b) != SPSP_OK) {   // (the words are checked here; the band itself needs the number of references)
                    cout << "-" << (char)ch << " takes a band of holder counts: " << spsp_last_error() << endl;
                    return 1;
                }
                select_each = ch == 'E';
                select_what = optarg;
                ++select_opts;
                break;
            }
            case 'l':
            case 'L':
                if (!parse_fraction(optarg, &tree_num, &tree_den, true)) {
                    cout << "-" << (char)ch << " takes a floor in [0, 1] with at most six digits behind the point, not '" << optarg << "'" << endl;
                    return 1;
                }
                tree_metric = ch == 'l' ? SPSP_CLUSTER_JACCARD : SPSP_CLUSTER_CONTAINMENT;
                ++tree_opts;
                break;
            case 'c':
            case 'C':
                if (!parse_fraction(optarg, &cluster_num, &cluster_den)) {
                    cout << "-" << (char)ch << " takes a threshold in (0, 1] with at most six digits behind the point, not '" << optarg << "'" << endl;
                    return 1;
                }
                cluster_metric = ch == 'c' ? SPSP_CLUSTER_JACCARD : SPSP_CLUSTER_CONTAINMENT;
                ++cluster_opts;
                break;
            case 'r':
            case 'R':
                if (!parse_fraction(optarg, &rep_num, &rep_den)) {
                    cout << "-" << (char)ch << " takes a threshold in (0, 1] with at most six digits behind the point, not '" << optarg << "'" << endl;
                    return 1;
                }
                rep_metric = ch == 'r' ? SPSP_CLUSTER_JACCARD : SPSP_CLUSTER_CONTAINMENT;
                ++rep_opts;
                break;
            case 'w': weights_file = optarg; break;
            case 'P':
                if (!parse_fraction(optarg, &pv_num, &pv_den)) {
                    cout << "-P takes a threshold in (0, 1] with at most six digits behind the point, not '" << optarg << "'" << endl;
                    return 1;
                }
                prevalence = true;
                break;
            case 'N': {
                char* e = nullptr;
                top = strtoll(optarg, &e, 10);
                if (e == optarg || *e || top < 1 || top > 64) { cout << "-N takes the number of neighbours listed per sketch, an integer in 1 .. 64, not '" << optarg << "'" << endl; return 1; }
                neighbours = true;
                break;
            }
            case 'J':
            case 'K':
            case 'I':
                if (!parse_fraction(optarg, &nb_num, &nb_den, true)) {
                    cout << "-" << (char)ch << " takes a threshold in [0, 1] with at most six digits behind the point, not '" << optarg << "'" << endl;
                    return 1;
                }
                nb_metric = ch == 'J' ? SPSP_NEIGHBOUR_JACCARD : ch == 'K' ? SPSP_NEIGHBOUR_CONTAINMENT : SPSP_NEIGHBOUR_CONTAINED;
                ++nb_opts;
                break;
            case 'f': inputfof = optarg; break;
            case 'q': query = optarg; break;
            case 'p': p = stoi(optarg); break;
            case 'm': min_threshold = stod(optarg); break;
            case 'o': output_name = optarg; break;
            case 'g': {
                char* e = nullptr;
                const long long v = strtoll(optarg, &e, 10);
                if (e == optarg || *e || v < 1) { cout << "-g takes the smallest number of new keys a reference is named for, an integer >= 1, not '" << optarg << "'" << endl; return 1; }
                gather = true; min_keys = (uint64_t)v;
                break;
            }
            case 's':
                if (string(optarg) == "auto") rate = SPSP_RATE_COARSEST;
                else {
                    char* e = nullptr;
                    rate = strtod(optarg, &e);
                    if (e == optarg || *e || !(rate > 0)) { cout << "-s takes a sampling rate > 0 or \"auto\", not '" << optarg << "'" << endl; return 1; }
                }
                break;
        }
    }
    if (cluster_opts > 1) { cout << "-c (Jaccard) and -C (containment) cluster the index: one of them, once" << endl; return 1; }
    if (cluster_opts && (query != "" || gather)) { cout << "-c / -C cluster the index all versus all: not together with -q or -g" << endl; return 1; }
    if (nb_opts > 1) { cout << "-J (Jaccard), -K (the larger containment) and -I (the row's containment) set the threshold of -N: one of them, once" << endl; return 1; }
    if (taxonomy && !classify) { cout << "-H gives the lineages of the index for the records of -X <records file>: it needs -X" << endl; return 1; }
    if (taxonomy && cf_top_seen) { cout << "-H assigns every record to one node of the tree: not together with -Y (-V and -I set its threshold)" << endl; return 1; }
    if (paired && !classify) { cout << "-x gives the mates of the records of -X <records file>, pair by pair: it needs -X" << endl; return 1; }
    if (extract && !classify) { cout << "-F names the records of -X <records file> to write out again: it needs -X" << endl; return 1; }
    if (split && !classify) { cout << "-j splits the records of -X <records file> into one file per reference or taxon: it needs -X" << endl; return 1; }
    if (split && extract) { cout << "-j writes every record and -F one subset of them: one of the two in a run" << endl; return 1; }
    if (split && spsp_split_word_check_host(split_what.c_str(), taxonomy ? 1 : 0) != SPSP_OK) { cout << "-j: " << spsp_last_error() << endl; return 1; }
    if (extract_plain && !extract && !split && !segments && !raw_coords) { cout << "-u writes the records of -F plain instead of gzipped: it needs -F" << endl; return 1; }
    if (extract && spsp_extract_word_check_host(extract_what.c_str(), taxonomy ? 1 : 0, 0xffffffffu) != SPSP_OK) { cout << "-F: " << spsp_last_error() << endl; return 1; }
    long long window_width = 0;
    string window_word;
    if (windows && !classify) { cout << "-y cuts the records of -X <records file> into windows and calls them stretch by stretch: it needs -X" << endl; return 1; }
    if (windows && (cf_top_seen || paired || extract || split)) {
        cout << "-y calls every window once and writes segments, not records: not together with -Y, -x, -F or -j" << endl;
        return 1;
    }
    if (windows) {
        char* e = nullptr;
        window_width = strtoll(window_arg.c_str(), &e, 10);
        if (e == window_arg.c_str() || (*e && *e != ':') || window_width < 1 || window_width > 0x7fffffffll) {
            cout << "-y takes <W>[:<word>], the window's width in bases, an integer in k .. 2147483647, and the call word, not '" << window_arg << "'" << endl;
            return 1;
        }
        window_word = *e == ':' ? string(e + 1) : string(taxonomy ? "taxon" : "best");
        if (spsp_windows_word_check_host(window_word.c_str(), taxonomy ? 1 : 0) != SPSP_OK) { cout << "-y: " << spsp_last_error() << endl; return 1; }
    }
    if (smooth && !windows) { cout << "-Q absorbs stray windows into the segments of -y <W>: it needs -y" << endl; return 1; }
    if (segments && !windows) { cout << "-Z writes segments of -y <W> out as FASTA: it needs -y" << endl; return 1; }
    if (raw_coords && !windows) { cout << "-O writes the segments of -y <W> in the coordinates of the records file as BED: it needs -y" << endl; return 1; }
    string segments_word;
    unsigned long long segments_min = 1;
    if (segments) {                                        // (<b> against the references: once they are counted, below)
        if (spsp_segments_word_check_host(segments_arg.c_str(), taxonomy ? 1 : 0, 0) != SPSP_OK) { cout << "-Z: " << spsp_last_error() << endl; return 1; }
        const size_t colon = segments_arg.find(':');
        segments_word = segments_arg.substr(0, colon);
        if (colon != string::npos) segments_min = strtoull(segments_arg.c_str() + colon + 1, nullptr, 10);
    }
    if (cf_opts && !classify) { cout << "-Y and -V belong to the classification of -X <records file>: they need -X" << endl; return 1; }
    if (classify && (query != "" || gather || cluster_opts || neighbours || prevalence || rep_opts || tree_opts || select_opts || accumulation || groups ||
                     (nb_opts && nb_metric != SPSP_NEIGHBOUR_CONTAINED))) {
        cout << "-X classifies the records of a sequence file against the index: not together with -q, -g, -c, -C, -N, -J, -K, -P, -r, -R, -l, -L, -S, -E, -A or -G" << endl;
        return 1;
    }
    const bool depth = !reads_files.empty();
    if (dp_min_seen && !depth) { cout << "-W belongs to the depth of -D <reads file>: it needs -D" << endl; return 1; }
    if (profile && !depth) { cout << "-B profiles the reads of -D <reads file> (which references they hold, each shared key counted once): it needs -D" << endl; return 1; }
    if (depth && (query != "" || gather || cluster_opts || neighbours || nb_opts || prevalence || rep_opts || tree_opts || select_opts || accumulation || groups || classify)) {
        cout << "-D counts how deep the reads of a sequence file cover the index: not together with -q, -g, -c, -C, -N, -J, -K, -I, -P, -r, -R, -l, -L, -S, -E, -A, -G or -X" << endl;
        return 1;
    }
    if (nb_opts && !neighbours && !classify) { cout << "-J / -K / -I set the threshold of the neighbour lists: they need -N (-I also serves -X)" << endl; return 1; }
    if (neighbours && (gather || cluster_opts)) { cout << "-N lists neighbours: not together with -g, -c or -C" << endl; return 1; }
    if (prevalence && (gather || cluster_opts || neighbours)) { cout << "-P counts the holders of every key: not together with -g, -c, -C or -N" << endl; return 1; }
    if (rep_opts > 1) { cout << "-r (Jaccard) and -R (containment) pick representatives of the index: one of them, once" << endl; return 1; }
    if (rep_opts && (cluster_opts || query != "" || gather || neighbours || prevalence)) {
        cout << "-r / -R pick representatives of the index all versus all: not together with -c, -C, -q, -g, -N or -P" << endl;
        return 1;
    }
    if (tree_opts > 1) { cout << "-l (Jaccard) and -L (containment) build the index's linkage tree: one of them, once" << endl; return 1; }
    if (tree_opts && (cluster_opts || query != "" || gather || neighbours || prevalence || rep_opts)) {
        cout << "-l / -L build the linkage tree of the index all versus all: not together with -q, -g, -c, -C, -N, -P, -r or -R" << endl;
        return 1;
    }
    if (select_opts > 1) { cout << "-S (one merged sketch) and -E (every sketch's own) write the selected keys: one of them, once" << endl; return 1; }
    if (select_opts && (gather || cluster_opts || neighbours || prevalence || rep_opts || tree_opts)) {
        cout << "-S / -E write sketches: not together with -g, -c, -C, -N, -P, -r, -R, -l or -L" << endl;
        return 1;
    }
    if (select_opts && !select_each && query != "") { cout << "-S writes the index's keys as one sketch: not together with -q (-E selects from the queries)" << endl; return 1; }
    if (acc_seeded && !accumulation) { cout << "-z seeds the orders of the accumulation curves: it needs -A" << endl; return 1; }
    if (accumulation && (query != "" || gather || cluster_opts || neighbours || prevalence || rep_opts || tree_opts || select_opts)) {
        cout << "-A draws the pan and core curves of the index: not together with -q, -g, -c, -C, -N, -P, -r, -R, -l, -L, -S or -E" << endl;
        return 1;
    }
    if (gp_opts && !groups) { cout << "-T, -U and -M belong to the groups of -G <labels file>: they need -G" << endl; return 1; }
    if (groups && (query != "" || gather || cluster_opts || neighbours || prevalence || rep_opts || tree_opts || select_opts || accumulation)) {
        cout << "-G counts the keys of the index's groups: not together with -q, -g, -c, -C, -N, -P, -r, -R, -l, -L, -S, -E or -A" << endl;
        return 1;
    }
    if (weights_file != "" && !rep_opts) { cout << "-w gives the weights -r / -R order the sketches by: it needs one of them" << endl; return 1; }
    vector<uint64_t> weights;
    if (weights_file != "" && inputfof != "") {
        vector<string> listed;
        if (!read_names(inputfof, listed)) return 1;
        string why;
        if (!read_weights(weights_file, listed.size(), weights, why)) { cout << "-w " << weights_file << ": " << why << endl; return 1; }
    }
    if (inputfof == "") {
        cout << "Core arguments:" << endl
             << "-f Index file of files (mandatory)" << endl
             << "-q Query file of files (\"\" for all versus all comparison of the index)" << endl
             << "-H Lineage file, one name;name;... line per index sketch: with -X <records file>, each record goes to the lowest common ancestor of its keys" << endl
             << "-F Records of -X <records file> to write out again as <prefix>_extract.fa.gz / .fq.gz: matched, unmatched, best=<j>, listed=<j>; with -H: classified, unclassified, taxon=<t>, clade=<t>" << endl
             << "-u Write the records of -F, or the files of -j, plain, not gzipped" << endl
             << "-j Split the records of -X <records file> into <prefix>_split_<b>.fa.gz / .fq.gz, one file per reference (best; the rest in _split_unmatched) or, with -H, per node (taxon, depth=<d>; the rest in _split_unclassified), and <prefix>_split.csv.gz; with -x <prefix>_split_<b>_1.* and _2.*; -u writes them plain" << endl
             << "-y <W>[:<word>] Windows: cut every record of -X <records file> into windows of W bases (overlapping by k - 1), call each as a record (best; with -H: taxon, depth=<d>) and write <prefix>_segments.csv.gz (stretches with one call) and <prefix>_mosaic.csv.gz (one line per record) in the place of the per-record CSVs; positions count the bases A, C, G, T only" << endl
             << "-Q <q> With -y: a run of at most q windows between two runs of one call, each longer than q windows, takes that call (its support counts as 0); 0 changes nothing" << endl
             << "-Z <what>[:<min_bases>] With -y: write the segments the word names (all, called, none, call=<b>, not=<b>, major, minor) of at least min_bases bases as <prefix>_segments.fa.gz, one FASTA record <name>:<begin + 1>-<end> per segment, 80 bases a line; -u writes it plain" << endl
             << "-O With -y: write the segments in the coordinates of the records file itself (counting N, IUPAC codes and lower case, as samtools faidx does) as <prefix>_segments.bed.gz: name, raw_begin, raw_end, call_name, 0, ., segment, begin, end, windows, support; -u writes it plain" << endl
             << "-x Mates file: with -X <records file>, record p of the two files is one pair, classified by the keys of both mates; -F then writes <prefix>_extract_1.* and <prefix>_extract_2.*" << endl
             << "Ouput arguments:" << endl
             << "-m Minimum value to be output (0.0)" << endl
             << "-p Required precision to be output in the CSV (6)" << endl
             << "-o output prefix (results)" << endl;
        return 0;
    }
    if (gather && query == "") { cout << "-g gathers the queries of -q against the index: it needs -q" << endl; return 1; }
    vector<string> names;
    uint32_t n_query = 0;
    if (query == "") {
        cout << "No query file, I will perform a all versus all comparison" << endl;
        read_names(inputfof, names);
        cout << "I found " << names.size() << " documents" << endl;
        n_query = (uint32_t)names.size();
    } else {
        read_names(query, names);
        n_query = (uint32_t)names.size();
        cout << "I query " << n_query << " file(s) against the bank" << endl;
        read_names(inputfof, names);
    }
    vector<const char*> paths;
    for (auto& s : names) paths.push_back(s.c_str());
    if (extract && !taxonomy && spsp_extract_word_check_host(extract_what.c_str(), 0, (uint32_t)paths.size()) != SPSP_OK) {   // (<j> against the list: no device yet)
        cout << "-F: " << spsp_last_error() << endl;
        return 1;
    }
    if (segments && !taxonomy && spsp_segments_word_check_host(segments_word.c_str(), 0, (uint32_t)paths.size() + 1) != SPSP_OK) {   // (likewise <b>)
        cout << "-Z: " << spsp_last_error() << endl;
        return 1;
    }
    // Devices: every visible GPU when there is enough work to split (the comparison is dealt by key over one context per
    // device, spsp_compare_files_multi), else the first.  SPSP_DEVICES="0,1,2,3" (or "0,0": two contexts on one device)
    // names them explicitly.  The reference has no such notion (one thread, Comparator.cpp:39-74).
    vector<int> devices;
    if (const char* e = getenv("SPSP_DEVICES")) {
        istringstream is(e);
        string tok;
        while (getline(is, tok, ',')) if (!tok.empty()) devices.push_back(atoi(tok.c_str()));
    }
    if (devices.empty()) {
        const int visible = spsp_device_count();
        if (visible <= 0) { cout << "GPU unavailable: " << spsp_last_error() << endl; return 1; }
        // sketches per device below which splitting does not pay (one partition + one exchange + a host join per device against
        // a comparison of a few hundred microseconds); SPSP_PER_DEVICE=<n> overrides the 512 (a guess until measured on a node)
        size_t per_device = 512;
        if (const char* e = getenv("SPSP_PER_DEVICE")) { const long v = atol(e); if (v > 0) per_device = (size_t)v; }
        const int use = (int)std::max<size_t>(1, std::min<size_t>((size_t)visible, names.size() / per_device));
        for (int d = 0; d < use; ++d) devices.push_back(d);
    }
    if (depth) {
        // one device, as -X (the driver opens a second context on it for the reads)
        vector<const char*> reads;
        for (auto& r : reads_files) reads.push_back(r.c_str());
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK && profile)
            rc = spsp_profile_files(ctx, paths.data(), (uint32_t)paths.size(), reads.data(), (uint32_t)reads.size(), (uint32_t)dp_min_count, (uint32_t)pf_min_keys, 0, (int)p,
                                    output_name.c_str(), 1, rate, nullptr, nullptr, nullptr, nullptr, nullptr);
        else if (rc == SPSP_OK)
            rc = spsp_depth_files(ctx, paths.data(), (uint32_t)paths.size(), reads.data(), (uint32_t)reads.size(), (uint32_t)dp_min_count, (int)p,
                                  output_name.c_str(), 1, rate, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << (profile ? "Profile failed: " : "Depth failed: ") << err << endl; return 1; }
        return 0;
    }
    if (classify) {
        // one device, as gather (the driver opens a second context on it for the records)
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK && windows && taxonomy)
            rc = spsp_taxonomy_files_raw(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), lineages_file.c_str(), (uint32_t)cf_min_keys, nb_num, nb_den,
                                         (int)p, output_name.c_str(), 1, rate, (uint64_t)window_width, window_word.c_str(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, (uint32_t)smooth_q, segments ? segments_word.c_str() : nullptr, segments_min, extract_plain ? 0 : 1, nullptr,
                                         nullptr, nullptr, raw_coords ? 1 : 0, nullptr, nullptr, nullptr);
        else if (rc == SPSP_OK && windows)
            rc = spsp_classify_files_raw(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), (uint32_t)cf_top, (uint32_t)cf_min_keys, nb_num, nb_den, (int)p,
                                         output_name.c_str(), 1, rate, (uint64_t)window_width, window_word.c_str(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, (uint32_t)smooth_q, segments ? segments_word.c_str() : nullptr, segments_min, extract_plain ? 0 : 1, nullptr,
                                         nullptr, nullptr, raw_coords ? 1 : 0, nullptr, nullptr, nullptr);
        else if (rc == SPSP_OK && split && taxonomy)
            rc = spsp_taxonomy_files_split(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), paired ? mates_file.c_str() : nullptr, lineages_file.c_str(),
                                           (uint32_t)cf_min_keys, nb_num, nb_den, (int)p, output_name.c_str(), 1, rate, split_what.c_str(), extract_plain ? 0 : 1, nullptr,
                                           nullptr, nullptr, nullptr);
        else if (rc == SPSP_OK && split)
            rc = spsp_classify_files_split(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), paired ? mates_file.c_str() : nullptr, (uint32_t)cf_top,
                                           (uint32_t)cf_min_keys, nb_num, nb_den, (int)p, output_name.c_str(), 1, rate, split_what.c_str(), extract_plain ? 0 : 1, nullptr,
                                           nullptr, nullptr, nullptr, nullptr);
        else if (rc == SPSP_OK && paired && taxonomy)
            rc = spsp_taxonomy_files_paired(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), mates_file.c_str(), lineages_file.c_str(), (uint32_t)cf_min_keys,
                                            nb_num, nb_den, (int)p, output_name.c_str(), 1, rate, extract ? extract_what.c_str() : nullptr, extract_plain ? 0 : 1, nullptr,
                                            nullptr, nullptr, nullptr);
        else if (rc == SPSP_OK && paired)
            rc = spsp_classify_files_paired(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), mates_file.c_str(), (uint32_t)cf_top, (uint32_t)cf_min_keys,
                                            nb_num, nb_den, (int)p, output_name.c_str(), 1, rate, extract ? extract_what.c_str() : nullptr, extract_plain ? 0 : 1, nullptr,
                                            nullptr, nullptr, nullptr, nullptr);
        else if (rc == SPSP_OK && taxonomy && extract)
            rc = spsp_taxonomy_files_extract(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), lineages_file.c_str(), (uint32_t)cf_min_keys, nb_num, nb_den,
                                             (int)p, output_name.c_str(), 1, rate, nullptr, nullptr, extract_what.c_str(), extract_plain ? 0 : 1, nullptr, nullptr);
        else if (rc == SPSP_OK && taxonomy)
            rc = spsp_taxonomy_files(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), lineages_file.c_str(), (uint32_t)cf_min_keys, nb_num, nb_den, (int)p,
                                     output_name.c_str(), 1, rate, nullptr, nullptr);
        else if (rc == SPSP_OK && extract)
            rc = spsp_classify_files_extract(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), (uint32_t)cf_top, (uint32_t)cf_min_keys, nb_num, nb_den, (int)p,
                                             output_name.c_str(), 1, rate, nullptr, nullptr, nullptr, extract_what.c_str(), extract_plain ? 0 : 1, nullptr, nullptr);
        else if (rc == SPSP_OK) rc = spsp_classify_files(ctx, paths.data(), (uint32_t)paths.size(), records_file.c_str(), (uint32_t)cf_top, (uint32_t)cf_min_keys, nb_num, nb_den,
                                                    (int)p, output_name.c_str(), 1, rate, nullptr, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << (taxonomy ? "Taxonomy failed: " : "Classification failed: ") << err << endl; return 1; }
        return 0;
    }
    if (groups) {
        // one device, as gather
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_groups_files(ctx, paths.data(), (uint32_t)paths.size(), labels_file.c_str(), (int)p, gp_num, gp_den, gp_onum, gp_oden,
                                                  gp_markers ? 1 : 0, output_name.c_str(), 1, rate, nullptr, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Groups failed: " << err << endl; return 1; }
        return 0;
    }
    if (accumulation) {
        // one device, as gather
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_accumulation_files(ctx, paths.data(), (uint32_t)paths.size(), (uint32_t)acc_orders, acc_seed, (int)p, output_name.c_str(), 1, rate,
                                                        nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Accumulation failed: " << err << endl; return 1; }
        return 0;
    }
    if (select_opts) {
        // one device, as gather; the rows of -E are every sketch of the index (n_query 0) or the queries
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_select_files(ctx, paths.data(), (uint32_t)paths.size(), query == "" ? 0u : n_query, select_what.c_str(), select_each ? 1 : 0,
                                                  output_name.c_str(), 1, rate, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Select failed: " << err << endl; return 1; }
        return 0;
    }
    if (tree_opts) {
        // one device, as gather
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_tree_files(ctx, paths.data(), (uint32_t)paths.size(), (int)p, tree_metric, tree_num, tree_den, output_name.c_str(), 1, rate,
                                                nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Linkage tree failed: " << err << endl; return 1; }
        return 0;
    }
    if (prevalence) {
        // one device, as gather; the rows are every sketch of the index (n_query 0) or the queries
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_prevalence_files(ctx, paths.data(), (uint32_t)paths.size(), query == "" ? 0u : n_query, (int)p, pv_num, pv_den,
                                                      output_name.c_str(), 1, rate, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Prevalence failed: " << err << endl; return 1; }
        return 0;
    }
    if (neighbours) {
        // one device, as gather
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_neighbours_files(ctx, paths.data(), (uint32_t)paths.size(), n_query, (int)p, nb_metric, nb_num, nb_den, (uint32_t)top,
                                                      output_name.c_str(), 1, rate, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Neighbours failed: " << err << endl; return 1; }
        return 0;
    }
    if (rep_opts) {
        // one device, as gather
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_representatives_files(ctx, paths.data(), (uint32_t)paths.size(), (int)p, rep_metric, rep_num, rep_den,
                                                           weights.empty() ? nullptr : weights.data(), output_name.c_str(), 1, rate, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Representatives failed: " << err << endl; return 1; }
        return 0;
    }
    if (cluster_opts) {
        // one device, as gather
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_cluster_files(ctx, paths.data(), (uint32_t)paths.size(), (int)p, cluster_metric, cluster_num, cluster_den, output_name.c_str(), 1,
                                                   rate, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Clustering failed: " << err << endl; return 1; }
        return 0;
    }
    if (gather) {
        // one device: the first of SPSP_DEVICES, else device 0
        spsp_ctx* ctx = nullptr;
        int rc = spsp_create(devices[0], nullptr, &ctx);
        if (rc == SPSP_OK) rc = spsp_gather_files(ctx, paths.data(), (uint32_t)paths.size(), n_query, (int)p, min_keys, 0, output_name.c_str(), 1, rate, nullptr, nullptr);
        const string err = rc != SPSP_OK ? spsp_last_error() : "";
        if (ctx) spsp_destroy(ctx);
        if (rc != SPSP_OK) { cout << "Gather failed: " << err << endl; return 1; }
        return 0;
    }
    // the progress lines of the reference (Comparator.cpp:56,69,364,414,503,509) are printed by the driver where the
    // reference prints them
    const int rc = spsp_compare_files_multi_rate(devices.data(), (uint32_t)devices.size(), paths.data(), (uint32_t)paths.size(), n_query, (int)p,
                                                 min_threshold, output_name.c_str(), query == "" ? 1 : 2, nullptr, rate);
    if (rc != SPSP_OK) { cout << "Comparison failed: " << spsp_last_error() << endl; return 1; }
    return 0;
}
