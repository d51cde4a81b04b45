// Internal declarations shared by the libspsp translation units (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/spsp.h"

namespace spsp {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define SPSP_HIP(call)                                                      \
    do {                                                                    \
        hipError_t _e = (call);                                             \
        if (_e != hipSuccess) return spsp::hip_fail(_e, #call, __FILE__, __LINE__); \
    } while (0)

// Grow-only device buffer owned by a context (re-used across calls so the
// steady state of a batch loop performs no hipMalloc).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);
    void release();
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// One candidate m-mer: hash <= threshold.  32 bytes.
struct Hit {
    uint64_t pos;    // absolute position of the m-mer in the concatenated bases
    uint64_t hash;   // XXH64(canonical m-mer, seed 1312)
    uint32_t canon;  // canonical 2-bit value
    uint32_t rec;    // record index
    uint32_t flags;  // bit0: occurrence is reverse strand; bit1: usable (inside a record of length >= k)
    uint32_t pad;
};

}  // namespace spsp

namespace spsp {
// HIP-event pairs recorded around one kind of launch
struct EventLog {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> used, spare;
};
// the events of one kind of record call (spsp_classify_device, spsp_taxonomy_device) while timing is on: in front of the probe, the
// route, the wave form, the workgroup form, and behind it; ms: their four spans added up since the pass's *_stage_ms call last read
// them.  mark(ctx, 0) opens a call (on: the context's timing as that call found it) and makes the events once; the context destroys them
struct RecordClock {
    hipEvent_t ev[5] = {};
    double ms[4] = {};
    bool on = false;
    int mark(spsp_ctx* ctx, int i);
    void hand_out(double* out4);          // -> out4, and ms cleared
};
enum { kEvDense = 0, kEvScan = 1, kEvAccumulate = 2, kEvCompare = 3, kEvScatter = 4, kEvGroup = 5, kEvKinds = 6 };
}  // namespace spsp

namespace spsp {
// a scan queued by scan_begin_impl and not yet collected by scan_end_impl
struct ScanJob {
    bool pending = false, empty = false;
    int redo_from = 0;           // first stage the next attempt runs: 0 dense, 1 compact (lists intact), 2 write pass
    bool segments = false;       // the attempt in flight is the scan by segments (spsp_stats.hip: thresholds that select nearly everything)
    bool use_bitmap = false;     // hit bitmap + k_expand (dense selections, list-overflow fallback) instead of per-wave lists
    bool lists = false;          // the attempt in flight used per-wave hit lists
    spsp_params p{};
    const uint8_t* d_bases = nullptr;
    uint64_t n_bases = 0, n_tiles = 0;
    const uint64_t* d_rec_off = nullptr;
    uint32_t n_rec = 0, hits_cap = 0, out_cap = 0;
    uint32_t n_lists = 0, list_cap = 0;   // geometry of the per-wave hit lists of the attempt in flight
    uint64_t rows_per_wave = 0;
};
struct CompareJob;   // spsp_compare.hip
// the key extraction queued by sketch_keys_begin_impl: what its last stages need when _end has to queue them (spsp_keys.hip)
struct KeysJob {
    bool has_hi = false, flat = false;   // flat: raw records by one lane per super-k-mer + per-genome LDS sort (the sorted form's kernels)
    uint32_t n_genomes = 0;
    uint64_t bound = 0;          // k-mer places of all genomes together (the extent of the staging arrays)
    uint32_t abundance = 1;
    bool big_queued = false;     // the table kernels for genomes beyond the LDS forms were queued by _begin
};
}  // namespace spsp

namespace spsp {
// spsp_ctx::h_scalar: the pinned uint64_t slots through which the kernel chains report to the host.  A slot is written by a
// kernel or an async copy queued on the context's stream and read by the host once it has waited for that work; a 32-bit value
// sits in the slot's low half.  A chain that needs one more word takes a free slot HERE.
enum HostSlot {
    kHsScanHits = 0,        // k_compact / k_expand / k_sum_counts / k_scan_top write the hit total (u64); scan_end_impl, scan_hits_impl read
    kHsSegEmitted = 0,      // ... the scan by segments instead: launch_scan_u32's total of super-k-mers (u64); scan_end_impl reads
    kHsScanEmitted = 1,     // k_resolve<true> writes the super-k-mers it emitted (u64); scan_end_impl reads
    kHsSegLeftTile = 1,     // ... the scan by segments instead: seg_scan_count copies the chains that left their tile (u32); scan_end_impl reads
    kHsScanFullest = 2,     // k_compact writes the fullest hit list (u64; k_compact reaches it from kHsScanHits), scan_enqueue zeroes it; scan_end_impl reads
    kHsStatChains = 3,      // count_superkmers_impl copies the chains that left their tile (u32) and reads it
    kHsIngestKept = 4,      // k_clean_scan / k_mixed_scan write the bases kept (u64); clean_device_impl / clean_mixed_impl read
    kHsIngestRecs = 5,      // ... and the records (u64), reached from kHsIngestKept: kIngestTotals slots in all
    kHsScanTotalA = 6,      // launch_scan_u32's total (u64) of gather_superkmers_impl (bases) and sketch_build_device_impl (places, then output bytes)
    kHsScanTotalB = 7,      // ... of sketch_build_device_impl (buckets, beside A's places), abundance_flags_impl (occurrences), the decoder and
                            // the key extraction (written, not read: they take the total from the scan's out[n])
    kHsCompareFlags = 8,    // 8..11: words [0, kFlags) of the comparison's flag block as uint32_t (spsp_compare.hip: compare_host_flags)
    kHsCells = 12,          // the cell count (u64) of a comparison returned as cells: copied behind the row sums (launch_accumulate_sparse) and
                            // read by compare_cells_run after compare_end_impl, or copied and read inside matrix_cells_impl
    kHsCellsBad = 12,       // spsp_matrix_add_cells_device copies k_matrix_add_cells' bad-cell word (u32) and reads it, in one call.  Shares the
                            // slot: compare_cells_run holds the context from its begin to its read, and the other two wait before they return.
                            // Nothing checks it: a caller must not add cells on a context between a cells comparison's begin and end
    kHsSlotsBad = 13,       // compare_slots_begin_impl copies k_slot_unpack's bad-record word (u32); slots_bad_record reads behind compare_end_impl
    kHsDownsampleTotal = 13,   // launch_scan_u32's total (u64) in keys_downsample_impl (written, never read).  Shares the slot: the drivers
                            // downsample (and wait) in front of the comparison they feed.  Nothing checks it: a downsampling pass queued on
                            // a context between a slot comparison's begin and end would overwrite that comparison's record check
    kHsOrderVerdict = 14,   // k_row_order's two u32 (sketches kept together in the new order | in the input's << 32); compare_end_impl reads
    kHsMultiVerdict = 15,   // k_parts_group's two u32 (records with a list | records sampled << 32), copied with the order verdict
    kHsClusterEdges = 16,   // spsp_cluster.hip: the copy of k_cl_link's edge count (u64); cluster_cells_impl reads behind its one wait
    kHsClusterBad = 17,     // ... of k_cl_link's bad-cell word (u32), in the same wait
    kHsClusterCount = 18,   // ... and launch_scan_u32's total over the "is a root" flags: the number of clusters (u64)
    kHsNbCands = 19,        // spsp_neighbours.hip: launch_scan_u32's total over the rows' passing partners: the candidates (u64)
    kHsNbRows = 20,         // ... its total over min(passing, top): the rows the call returns (u64)
    kHsNbPairs = 21,        // ... the copy of k_nb_count's count of cells with a passing end (u64)
    kHsNbBad = 22,          // ... and of its bad-cell word (u32): neighbours_cells_impl reads all four behind its first wait
    kHsPvBad = 23,          // spsp_prevalence.hip: the copy of the count / read-back kernels' two u32 (keys out of order | a probe sequence
                            // that went round the table << 32); prevalence_device_impl reads it behind its one wait
    kHsRpUndecided = 24,    // spsp_representatives.hip: the copy of the sketches still undecided behind a batch of rounds (u32), queued behind
                            // the batch; representatives_cells_impl reads it behind that batch's wait
    kHsRpEdges = 25,        // ... of k_rp_edges' edge count (u64), in the same wait: sizes the later batches' grids, and is *n_edges
    kHsRpBad = 26,          // ... and of two u32 (k_rp_edges' bad-cell word | the round that decided the last sketch << 32), in the same wait
    kHsRpCount = 27,        // ... launch_scan_u32's total over the "is its cluster's first member" flags: the representatives (u64);
                            // representatives_cells_impl reads it behind its last wait
    kHsTrEdges = 28,        // spsp_tree.hip: the copy of the candidate-edge count k_tr_pick's first round wrote down (u64)
    kHsTrBad = 29,          // ... of two u32 (k_tr_edges' bad-cell word | the forest's edge count << 32)
    kHsTrRounds = 30,       // ... and of the rounds that hooked anything (u32): tree_cells_impl reads all three behind its one wait
    kHsSelBad = 31,         // spsp_select.hip: the copy of the table fill's two u32 (keys out of order | a probe sequence that went round
                            // the table << 32); keys_select_impl reads it behind its first wait
    kHsSelTotal = 32,       // ... and launch_scan_u32's total over the tiles' survivor counts: the keys selected (u64), in the same wait
    kHsAcBad = 33,          // spsp_accumulation.hip: the copy of two u32 (the table fill's keys out of order | a probe sequence that went round
                            // the table or a list place out of range << 32); accumulation_device_impl reads it behind its one wait
    kHsGpBad = 34,          // spsp_groups.hip: the copy of the first table fill's two u32 (keys out of order | a probe sequence that went round
                            // the table << 32); groups_device_impl reads it behind its first wait
    kHsGpCell = 35,         // ... of the cell table's word (u32: a probe sequence that went round it, or an entry without its cell), in the same wait
    kHsGpTotal = 36,        // ... and launch_scan_u32's total over the tiles' survivor counts: the marker keys of all groups (u64), in the same wait
    kHsCfBad = 37,          // spsp_classify.hip: the copy of two u32 (the index build's keys out of order | a probe sequence that went round
                            // the table or a list place out of range << 32) behind the index call's wait; behind a classify call's one
                            // wait the copy of its own word (u32: a record routed to a form its work does not fit)
                            // -- and behind a taxonomy call's one wait (spsp_taxonomy.hip) the copy of that call's word, the same way
    kHsUnBad = 38,          // spsp_union.hip: the copy of k_un_flag's word (u64: ~0, or the least side << 32 | record whose keys do not
                            // ascend strictly); records_union_impl reads it behind its one wait
    kHsUnNew = 39,          // ... and launch_scan_u32's total over the tiles' counts: the keys of B that A does not hold (u64), in the same wait
    kHostSlots = 40
};
constexpr int kIngestTotals = 2;
static_assert(kHsIngestKept + kIngestTotals <= kHsScanTotalA, "the ingest totals end in front of the scan totals");
static_assert(kHsIngestRecs == kHsIngestKept + 1 && kHsMultiVerdict == kHsOrderVerdict + 1 && kHsMultiVerdict < kHostSlots, "slots reached from their neighbour");
static_assert(kHsNbCands == kHsClusterCount + 1 && kHsPvBad == kHsNbBad + 1 && kHsPvBad + 1 == kHsRpUndecided, "the neighbours' four slots, then the prevalence pass's one");
static_assert(kHsRpCount == kHsRpUndecided + 3 && kHsRpCount + 1 == kHsTrEdges, "the representatives pass's four slots, then the linkage tree's");
static_assert(kHsTrRounds == kHsTrEdges + 2 && kHsTrRounds + 1 == kHsSelBad, "the linkage tree's three slots");
static_assert(kHsSelTotal == kHsSelBad + 1 && kHsSelTotal + 1 == kHsAcBad, "the selection's two slots");
static_assert(kHsAcBad + 1 == kHsGpBad, "the accumulation's one slot");
static_assert(kHsGpCell == kHsGpBad + 1 && kHsGpTotal == kHsGpBad + 2 && kHsGpTotal + 1 == kHsCfBad, "the groups pass's three slots");
static_assert(kHsCfBad + 1 == kHsUnBad && kHsUnNew == kHsUnBad + 1 && kHsUnNew + 1 == kHostSlots, "the classification's one slot, then the union's two: the last ones");
// ctx->c_flags (spsp_compare.hip names its words): the two words behind those a comparison's kernels use hold the cell count (u64)
// of a comparison returned as cells (spsp_multi.hip)
constexpr uint32_t kCfCellCount = 14;
// ... and behind those, two words of the key extraction (spsp_keys.hip names them): no clearing kernel of a comparison reaches them
constexpr uint32_t kCfKeysFlags = 16;
}  // namespace spsp

struct spsp_ctx {
    bool timing = false;          // any kind enabled
    uint32_t timing_mask = 0;     // bit k: regions of kind k (kEvDense ...) are bracketed by events
    spsp::EventLog evlog[spsp::kEvKinds];
    // begin/end bracket for one timed region; no-ops unless timing is on
    int ev_begin(int kind);
    int ev_end(int kind);
    bool ev_pair(int kind, hipEvent_t* start, hipEvent_t* stop);   // events for hipExtLaunchKernelGGL (no stream packets)
    bool ev_open[spsp::kEvKinds] = {};   // a begin without its end is outstanding
    uint32_t timing_every = 1;           // spsp_timing_sample: every n-th region of a kind is bracketed
    uint32_t ev_seq[spsp::kEvKinds] = {};
    spsp_stage_times stages{};    // whole-file drivers: wall seconds per stage (spsp_stage_times_read)
    int device = 0;
    int n_cu = 256;          // compute units this context's stream may use (spsp_set_cu_count)
    int n_cu_device = 256;   // ... of the device
    int dense_blocks_per_cu = 1;   // table variants of the dense pass: 1024-lane workgroups per CU (spsp_set_cu_count)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t tail_stream = nullptr;   // sparse stages of the scan (spsp_scan_tail_stream); nullptr = the main stream
    bool own_tail_stream = false;
    hipStream_t sparse_stream() const { return tail_stream ? tail_stream : stream; }
    uint64_t* h_scalar = nullptr;  // pinned, spsp::kHostSlots slots: what each holds is spsp::HostSlot
    hipEvent_t dense_done = nullptr;   // recorded behind every dense pass (unless a timing event already is)
    hipEvent_t dense_marker = nullptr; // what spsp_wait_dense waits on
    hipEvent_t tail_event = nullptr;   // spsp_wait_stream: marks the current end of this context's stream
    hipEvent_t scan_done = nullptr;    // behind the last kernel of the queued scan: what spsp_scan_device_end waits on
    hipEvent_t compare_done = nullptr; // likewise for the queued comparison
    uint64_t learnt_on = 0;            // offsets' fingerprint of the collection order_quiet / multi_quiet were learnt on
    uint32_t multi_quiet = 0;          // comparisons that leave out the has-a-list bits (the last one had lists for most records)
    uint32_t order_quiet = 0;          // comparisons that skip the making of a row order (the last one came in a good order of its own)
    std::vector<const void*> lds_kernels;   // kernels whose dynamic-LDS limit this context has raised (lds_opt_in)
    spsp::ScanJob scan_job;
    spsp::CompareJob* compare_job = nullptr;
    // spsp_sketch_keys_device_begin / _end (spsp_keys.hip)
    bool keys_pending = false, keys_has_hi = false, keys_flags_clear = false;
    bool keys_unordered = false;       // spsp_compare_keys_unordered: the comparisons of this context do not insist on sorted sketches
    uint32_t keys_genomes = 0;
    bool keys_sorted = false;          // the pending extraction promised sorted sketches (its big genomes are sorted in _end)
    // a comparison whose caller wants the pair matrix as sparse cells (spsp_multi.hip: compare_cells_run)
    struct CellsReq { unsigned long long* cells = nullptr; unsigned long long cap = 0; unsigned long long* count = nullptr; bool armed = false, direct = false; } cells_req;
    spsp::KeysJob keys_job;
    bool keys_expect_big = false;      // the last extraction collected on this context met a genome beyond the LDS forms
    uint32_t keys_big_genomes = 0;     // genomes of the last collected extraction that went through the global-memory stages (spsp_bigkeys.hip)
    hipEvent_t keys_done = nullptr;
    uint32_t* h_keys = nullptr;        // pinned: genome record ranges in, key offsets + overflow report out
    size_t h_keys_cap = 0;
    uint8_t* h_text = nullptr;         // pinned staging for a whole FASTA file (spsp_sketch_file reads plain files straight into it)
    size_t h_text_cap = 0;
    uint64_t* h_skoff = nullptr;       // pinned staging for the sketch offsets of a queued comparison
    size_t h_skoff_cap = 0;
    struct ReadRegion { uint8_t* p = nullptr; size_t cap = 0; };
    std::vector<ReadRegion> h_read_regions;   // spsp_compare_files: one per reader thread, the payloads of its files back to back (kept: page faults and munmaps per call otherwise)
    // scan workspace
    spsp::DevBuf bases, rec_off, bitmap, tile_count, tile_off, hits, emit_count, scan_tmp, d_scalar, seg_a, seg_b;
    spsp::DevBuf wave_hits, wave_cnt;    // per-wave hit lists of the table variants of the dense pass
    spsp::DevBuf packed, unpacked;       // SPSP_SCAN_PACKED_INPUT: spsp_pack_bases_device's output; ASCII copy for the variants that need one
    spsp::DevBuf st_count, st_open, st_total, st_over;      // print_stat counting pass (spsp_stats.hip)
    uint64_t hits_cap = 0, out_cap = 0;  // entries the sparse-stage buffers of the call in flight are sized for (grow on overflow)
    // what the last overflow taught: hits / super-k-mers per base at that threshold (scan_begin_impl sizes the next call by it)
    bool learn_valid = false;
    uint64_t learn_threshold = 0;
    double learn_hits_per_base = 0, learn_out_per_base = 0;
    uint64_t list_cap = 0;               // hits one wave's list holds (grows on overflow)
    uint64_t list_cap_threshold = 0;     // ... learnt at this threshold (another threshold starts from its own expectation)
    // LDS pre-filter table cache (keyed by m, threshold)
    spsp::DevBuf filter;
    uint32_t filter_m = 0;
    uint64_t filter_thr = 0;
    uint32_t filter_shift = 0;
    bool filter_valid = false;
    // blocked Bloom filter over canonical m-mers (k_dense_bloom)
    spsp::DevBuf bloom;
    uint32_t bloom_m = 0;
    uint64_t bloom_thr = 0;
    bool bloom_valid = false;
    // pair-lookup table cache (64 KiB table + 8 KiB key bitmap)
    spsp::DevBuf pairtab;
    uint32_t pair_m = 0;
    uint64_t pair_thr = 0;
    bool pair_valid = false;
    // ingest workspace (GPU-side getLineFasta + clean_dna)
    spsp::DevBuf i_text, i_tiles, i_entry, i_outoff, i_recbase, i_lens, i_dst, i_compact;
    spsp::DevBuf i_tinfo, i_dbase, i_fqbad;   // FASTQ / mixed batches: tile words, D at every tile, first malformed record per file
    // compare workspace
    spsp::DevBuf c_min, c_lo, c_hi, c_table, c_owner, c_rowid, c_row, c_matrix, c_inter, c_flags, c_skoff, c_slot_lo, c_slot_hi, c_slot_mn, c_part_cnt, c_recs, c_where, c_lref, c_filter, c_bits, c_sig, c_order, c_multi, scan_blocks;
    uint64_t spill_expect = 0;     // records the last unfiltered partition-form comparison had in overflowed parts (0: none) -- see spill_plan
    uint32_t filter_skipped = 0;
    double filter_ratio = 1.0;   // records dealt into parts per owned key in the last filtered comparison (sizes the next one's parts)
    spsp::DevBuf x_cnt, x_off, x_begin, x_end, x_tot;   // key-partitioned exchange (spsp_compare.hip)
    spsp::DevBuf bl_hist, bl_keys, bl_vals, bl_meta, bl_lo, bl_hi, bl_pmin, bl_pb, bl_slot, bl_first, bl_codes, bl_text, bl_outs, bl_out, bl_sk;   // sketch builder on the device (spsp_build.hip; bl_sk: the stream spsp_sketch_build_device uploads)
    spsp::DevBuf dc_text, dc_desc, dc_mn, dc_lo, dc_hi, dc_meta, dc_walk;   // bulk sketch decode (spsp_decode.hip)
    spsp::DevBuf a_cnt, a_off, a_mn, a_lo, a_hi, a_slot, a_slot_of, a_flags, a_seg;   // -a abundance pass (spsp_abund.hip)
    // genomes / sketches beyond the per-segment LDS forms (spsp_bigkeys.hip): output slices, the open-addressing table in HBM
    // (slot words carry the epoch of the call that claimed them: never cleared between calls), the sort's tile list
    spsp::DevBuf b_mn, b_lo, b_hi, b_table, b_tiles, b_seg;
    std::vector<uint64_t> m_h_skoff;                          // host arrays a queued slot unpack reads (spsp_multi.hip)
    std::vector<uint32_t> m_h_tot, m_h_base;
    bool m_slots_job = false;                                 // the pending comparison came from exchange slots: its record check is read behind compare_end
    spsp::DevBuf m_send, m_recv, m_cells, m_mn, m_lo, m_hi;   // key-partitioned split (spsp_multi.hip): slots out / in, sparse cells, unpacked keys
    uint32_t big_epoch = 0;
    // key downsampling (spsp_downsample.hip): two sets of output arrays used in turn (ds_flip: the set the next call fills), work area
    spsp::DevBuf ds_mn[2], ds_lo[2], ds_hi[2], ds_work;
    int ds_flip = 0;
    // gather (spsp_gather.hip): sketch offsets, per-(query, reference) counters / their scan / fill places, per-query-key counts
    // (the rounds' dead flags) / their scan, edge list, edges by reference, holders by query key, counters, round state, a batch's rows
    spsp::DevBuf g_off, g_u, g_roff, g_rfill, g_qcnt, g_qoff, g_edges, g_byref, g_hold, g_count, g_state, g_rows;
    // clustering (spsp_cluster.hip): the per-sketch arrays and the counter words in one work area, the rows
    spsp::DevBuf cl_work, cl_rows;
    // neighbours (spsp_neighbours.hip): the per-row arrays and the counter words in one work area, the candidate list, the rows
    spsp::DevBuf nb_work, nb_cand, nb_rows;
    // prevalence (spsp_prevalence.hip): sketch offsets, the key table in HBM (one 64-bit word per slot: claimer | counter << 32), h of
    // every key occurrence, the rows, the flag words with the spectrum behind them
    spsp::DevBuf pv_off, pv_table, pv_hold, pv_rows, pv_spec;
    uint32_t pv_log2cap = 0;             // slots of the table the last prevalence call used, as a power of two
    // representatives (spsp_representatives.hip): the per-sketch arrays and the counter words in one work area, the edge list (one
    // 32-bit word per link, room for one per cell), the rows
    spsp::DevBuf rp_work, rp_edges, rp_rows;
    // linkage tree (spsp_tree.hip): the per-sketch arrays and the counter words in one work area, the two lists of live edges (one
    // cell word per candidate, room for one per cell in each), the forest's cell words
    spsp::DevBuf tr_work, tr_edges, tr_forest;
    // selection (spsp_select.hip): two sets of output arrays used in turn (sel_flip: the set the next call fills -- the result of one
    // call may be the input of the next), the merged form's sort scratch, and the work area (flag words, keep mask, offsets, tile counts)
    spsp::DevBuf sel_mn[2], sel_lo[2], sel_hi[2], sel_t_mn, sel_t_lo, sel_t_hi, sel_work;
    int sel_flip = 0;
    // accumulation (spsp_accumulation.hip): the work area (flag words, the two scans' inputs and outputs), the key-major form (a start
    // per distinct key and one more; the holders' sketch numbers, 16 bits each, list behind list), the orders as rank tables, and the two
    // histograms (first rank, mex) of every order
    spsp::DevBuf ac_work, ac_keys, ac_list, ac_rank, ac_hist;
    // groups (spsp_groups.hip): the cell table in HBM (one 64-bit word per slot: claimer | group << 32 | counter << 48), one word per
    // key occurrence (h_c and the key's properties for the entry's group), the work area (flag words, the sketches' groups, the
    // groups' bounds, the per-sketch records, keep mask, offsets, tile counts, destinations), the marker keys, and the compaction's
    // output, which is the sort's scratch afterwards
    spsp::DevBuf gp_table, gp_cell, gp_work, gp_mn, gp_lo, gp_hi, gp_t_mn, gp_t_lo, gp_t_hi;
    // classification (spsp_classify.hip).  The index IS the prevalence table (pv_table, its counters spent as cursors) and the
    // accumulation's key-major form (ac_work: key_no per entry; ac_keys: key_start; ac_list) over the caller's reference arrays:
    // whatever fills that table again (prevalence_fill_table) drops it.  Per record call, classify's or taxonomy's (RecordWork; every
    // call waits for the device before it returns, so nothing is in use across calls): record offsets, key number + 1 per record
    // key, work and hit keys per record, the two queues with their counters and the flag word, the records' rows (four words for
    // classify, eight for taxonomy), and the counter rows of either workgroup form where they do not fit the LDS; classify's hits
    struct ClassifyIndex {
        bool valid = false, has_hi = false;
        uint32_t n_ref = 0, entries = 0;
        uint64_t first = 0;
        const uint32_t* mn = nullptr;
        const uint64_t *lo = nullptr, *hi = nullptr;
        const uint32_t *key_no = nullptr, *key_start = nullptr;
        const uint16_t* list = nullptr;
        bool depth = false;               // spsp_depth_begin_device has made counters for THIS index: they end with it
        uint32_t distinct = 0;            // ... and read D, its distinct keys
        std::vector<uint64_t> off_host;   // the references' offsets as the index call got them (n_ref + 1)
        bool taxonomy = false;            // spsp_taxonomy_index_device has attached a tree to THIS index: it ends with it
        uint32_t tx_nodes = 0;            // ... of T nodes
    } cf_index;
    spsp::DevBuf cf_off, cf_kn, cf_work, cf_queue, cf_rec, cf_hits, cf_rows;
    // depth (spsp_depth.hip): one 32-bit counter per distinct key of the index; per index entry its key's number and whether that
    // key is unique (made once, by begin), and its key's count (made by every read, handed out); the rows; the two total words
    // (hit keys since begin | the index keys found at the last read)
    spsp::DevBuf dp_count, dp_kn, dp_uniq, dp_entry, dp_rows, dp_words;
    spsp::DevBuf dp_long, dp_hist;       // the long references and their segments (made by begin); their sums and histograms in device memory (per read)
    uint32_t dp_n_long = 0, dp_n_seg = 0;
    uint64_t dp_record_keys = 0;         // record keys added since begin
    std::vector<std::pair<hipEvent_t, hipEvent_t>> dp_add_used, dp_add_spare;   // while timing is on: a pair around every add's launch, read by spsp_depth_stage_ms
    hipEvent_t dp_events[3] = {};        // ... and in front of a read's entry pass, of its reduction, and behind it
    double dp_ms[3] = {};                // the milliseconds added up since spsp_depth_stage_ms last read them: add, entry, reduce
    // profile (spsp_profile.hip), on the depth counters: the live-key counter per reference, a dead byte per distinct key, an
    // assigned byte per index entry, the state words of the rounds, a batch's round records, the reduced rows
    spsp::DevBuf pf_u, pf_dead, pf_assigned, pf_state, pf_rounds, pf_rows;
    std::vector<hipEvent_t> pf_events;   // while timing is on: around the start, every pick and walk of a batch, and the reduction
    double pf_ms[4] = {};                // ... their milliseconds since spsp_profile_stage_ms last read them: start, picks, walks, reduction
    uint32_t pf_last[3] = {};            // the last call's rounds queued, rows and host waits (spsp_profile_counts hands them out)
    // which form answered (spsp_stats_counts hands them out): the last collected scan's form (0 none or empty, 1 by segments, 2 the
    // product scan, 3 the product scan after the segment count left a chain unfinished) and its kHsSegLeftTile; the last
    // super-k-mer count's form (1 k_seg_count + k_seg_tail, 2 the chunk kernels from the start, 3 after a hand-over) and its kHsStatChains
    uint32_t st_last[4] = {};
    // taxonomy (spsp_taxonomy.hip), on the classification's index: the tree (parent | size | ref_node), node(x) per distinct key,
    // the same per index entry where it was asked for.  Its calls work in the classification's per-call arrays above
    spsp::DevBuf tx_tree, tx_key_node, tx_entry_node;
    spsp::RecordClock cf_clock, tx_clock;   // spsp_classify_stage_ms, spsp_taxonomy_stage_ms
    // extraction (spsp_extract.hip): the call's words, the tiles' sums and their scan (the text's tiles, then the records'), the
    // records' starts, the keep flags, the run table (output starts, then source starts) and the output, which is whole stretches
    spsp::DevBuf ex_words, ex_tiles, ex_bases, ex_begin, ex_keep, ex_runs, ex_out;
    hipEvent_t ex_ev[4] = {};            // while timing is on: in front of the starts, the offsets, the copy, and behind it
    uint32_t ex_marked = 0;              // ... which of them the call in flight has recorded
    double ex_ms[3] = {};                // their milliseconds since spsp_extract_stage_ms last read them: starts, offsets, copy
    // split (spsp_split.hip), in the extraction's words, tiles, starts and output: the records' bins, the run table (the runs'
    // prefix of kept bytes and source starts in record order, the sort's keys and values twice, the sorted runs' source and output
    // starts), and the bins' offsets
    spsp::DevBuf sp_bin, sp_runs, sp_off;
    hipEvent_t sp_ev[6] = {};            // while timing is on: in front of the starts, the runs, the order, the offsets, the copy, and behind it
    uint32_t sp_marked = 0;
    double sp_ms[5] = {};                // spsp_split_stage_ms: starts, runs, order, offsets, copy
    // union of two record batches (spsp_union.hip): the output arrays, and the work area (the flag word, the three offset arrays,
    // a place in A per entry of B, the "new" ballot words of B's entries, the tiles' counts and their scan)
    spsp::DevBuf un_mn, un_lo, un_hi, un_work;
    spsp::RecordClock un_clock;          // spsp_union_stage_ms: flag, scan, offsets, write
    // windows (spsp_windows.hip): the call's words, the tiles' sums and their scan, per record its first window and output start,
    // the windows' offsets, their source starts, and the output, which is whole stretches with the scan's readable bytes behind
    spsp::DevBuf wn_words, wn_tiles, wn_rec, wn_off, wn_src, wn_out;
    hipEvent_t wn_ev[4] = {};            // while timing is on: in front of the count, the offsets, the copy, and behind it
    double wn_ms[3] = {};                // spsp_windows_stage_ms: count, offsets, copy
    // segments as sequence (spsp_segments.hip): the call's upload (the three tables and the headers) and the text, whole stretches
    spsp::DevBuf sg_tab, sg_out;
    std::vector<uint8_t> sg_host;        // the upload's host copy: it stays until the next call, as the copy may still read it
    hipEvent_t sg_ev[2] = {};            // while timing is on: in front of the launch and behind it
    bool sg_marked = false;
    double sg_ms = 0;                    // spsp_segments_stage_ms: the write
    // raw coordinates (spsp_lift.hip): the tiles' summaries, their entry states, the prefixes K | S | R (n_tiles + 1 each), the
    // uploaded indices, the work arrays (sequence rank, record and record start per query, then every record's start) and the
    // outputs (raw, the lengths, the records as 32-bit words)
    spsp::DevBuf lf_tiles, lf_entry, lf_pre, lf_q, lf_work, lf_out;
    hipEvent_t lf_ev[4] = {};            // while timing is on: in front of the count, the scan, the answer, and behind it
    double lf_ms[3] = {};                // spsp_lift_stage_ms: count, scan, answer
};

namespace spsp {
// more dynamic LDS than the default limit allows: hipFuncSetAttribute(MaxDynamicSharedMemorySize), once per kernel and context (spsp_abi.hip)
int lds_opt_in(spsp_ctx* ctx, const void* kernel, size_t bytes);
template <class... A> int lds_opt_in(spsp_ctx* ctx, void (*kernel)(A...), size_t bytes) { return lds_opt_in(ctx, reinterpret_cast<const void*>(kernel), bytes); }
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// scan pipeline (spsp_scan.hip)
int scan_device_impl(spsp_ctx* ctx, const spsp_params* p, const uint8_t* d_bases, uint64_t n_bases,
                     const uint64_t* d_rec_off, uint32_t n_rec, spsp_superkmer** d_out, uint64_t* n_out);
int scan_begin_impl(spsp_ctx* ctx, const spsp_params* p, const uint8_t* d_bases, uint64_t n_bases,
                    const uint64_t* d_rec_off, uint32_t n_rec);
int scan_end_impl(spsp_ctx* ctx, spsp_superkmer** d_out, uint64_t* n_out);
int seg_scan_count(spsp_ctx* ctx, const spsp_params* p, const uint8_t* d_bases, bool packed, uint64_t n_bases, const uint64_t* d_rec_off, uint32_t n_rec);
int seg_scan_emit(spsp_ctx* ctx, const spsp_params* p, const uint8_t* d_bases, bool packed, uint64_t n_bases, const uint64_t* d_rec_off, uint32_t n_rec,
                  spsp_superkmer* d_out, uint64_t out_cap);
int scan_hits_impl(spsp_ctx* ctx, const spsp_params* p, const uint8_t* d_bases, uint64_t n_bases,
                   uint64_t* n_hits);
// compare pipeline (spsp_compare.hip)
int compare_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_min, const uint64_t* d_lo,
                        const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n, uint32_t row_limit, uint32_t row_first,
                        uint32_t row_stride, uint32_t* d_inter);
int compare_device_begin_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_min, const uint64_t* d_lo,
                              const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n, uint32_t row_limit,
                              uint32_t row_first, uint32_t row_stride, uint32_t* d_inter);
int compare_end_impl(spsp_ctx* ctx);
void compare_job_drop(spsp_ctx* ctx);
int check_params(const spsp_params* p);
int pack_bases_impl(spsp_ctx* ctx, const uint8_t* d_bases, uint64_t n_bases, uint32_t** d_packed);
// every super-k-mer of the input, selected or not (spsp_stats.hip)
// packed: d_bases holds 2-bit words (16 bases per dword); base0: first base of rec_off[0]'s record in d_bases, added to every offset
int count_superkmers_impl(spsp_ctx* ctx, const spsp_params* p, const uint8_t* d_bases, uint64_t n_bases, const uint64_t* d_rec_off,
                          uint32_t n_rec, uint64_t* total, bool packed = false, uint64_t base0 = 0, const uint32_t* h_file_rec = nullptr, uint32_t n_files = 1);
// bulk sketch decode (spsp_decode.hip): one stored super-k-mer of a sketch payload, as the host's structure walk finds it
struct DecDesc {
    uint64_t off;    // byte offset in the payload (later: in the concatenated payload buffer): blob bytes (kind 0) / prefix line (kind 1)
    uint32_t mn;     // minimizer of the bucket (2-bit value)
    uint32_t info;   // bits 0-1 kind: 0 maximal super-k-mer in the blob, 1 "prefix\nsuffix\n" pair, 2 the bare minimizer (k == m);
                     // kind 1: prefix length bits 2-9, suffix length bits 10-17
    uint32_t out;    // first raw key of this super-k-mer
    uint32_t pad;
};
struct ParsedSketch {
    uint32_t k = 0, m = 0;
    bool standard = true;        // laid out as the sketcher writes it: the GPU path applies
    uint64_t n_keys = 0;         // raw keys (duplicates included)
    std::vector<DecDesc> desc;   // offsets relative to the payload; `out` relative to the sketch
};
// structure of one payload: header + bucket boundaries + line ends (spsp_host.cpp: pure host code, fuzzed under ASan)
int sketch_parse_structure_host(const uint8_t* payload, uint64_t len, ParsedSketch* P);
// spsp_downsample.hip: the keys whose minimizer's hash is <= threshold, sketches back to back, order kept, in context-owned arrays
int keys_downsample_impl(spsp_ctx* ctx, uint32_t k, uint64_t threshold, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi,
                         const uint64_t* h_sk_off, uint32_t n, uint32_t** out_mn, uint64_t** out_lo, uint64_t** out_hi, uint64_t* sk_off_out);
// the tile compaction behind a keep mask, shared by the downsampling pass, the selection and the groups pass (spsp_downsample.hip).  The mask is
// k_ds_flag's layout: tiles of kDsTile keys, one 64-bit ballot word per 64 keys -- round r of wave w of tile t fills word
// kDsWords t + 4 r + w, bit l of word j is key 64 j + l -- and d_tile_cnt[t] = the tile's survivors.  Queued on the context's stream:
// launch_scan_u32 over the tile counts (d_tile_off: n_tiles + 1 words, the last the total, also stored to *total_host), k_ds_move
// (the kept keys of (d_mn, d_lo, d_hi), order kept, to (out_mn, out_lo, out_hi)), k_ds_offsets (d_off_out[i] = the survivors in
// front of key d_off_in[i], n_bounds of them).  No host wait.
constexpr uint32_t kDsThreads = 256;                       // 4 waves
constexpr uint32_t kDsTile = 2048;                         // keys per workgroup: 8 rounds of 256
constexpr uint32_t kDsWords = kDsTile / 64;                // ballot words per tile
int ds_compact_launch(spsp_ctx* ctx, bool has_hi, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const unsigned long long* d_mask,
                      const uint32_t* d_tile_cnt, uint32_t* d_tile_off, uint32_t n_tiles, const uint64_t* d_off_in, uint32_t n_bounds, uint64_t* d_off_out,
                      uint32_t* out_mn, uint64_t* out_lo, uint64_t* out_hi, uint64_t* total_host);
// the compaction's part of a work area, written once: keep mask | offsets in | offsets out | tile counts | tile offsets (+ the total).
// base: 8-byte aligned, bytes() of room behind it
struct DsWork {
    unsigned long long* mask;
    uint64_t *off_in, *off_out;
    uint32_t *tile_cnt, *tile_off;
    static size_t bytes(uint32_t n_tiles, uint32_t n_bounds) { return (size_t)n_tiles * kDsWords * 8 + (size_t)2 * n_bounds * 8 + ((size_t)2 * n_tiles + 2) * 4 + 64; }
    DsWork(void* base, uint32_t n_tiles, uint32_t n_bounds)
        : mask(reinterpret_cast<unsigned long long*>(base)), off_in(reinterpret_cast<uint64_t*>(mask + (size_t)n_tiles * kDsWords)), off_out(off_in + n_bounds),
          tile_cnt(reinterpret_cast<uint32_t*>(off_out + n_bounds)), tile_off(tile_cnt + n_tiles) {}
};
// flag, then compact: what the selection and the groups pass do with one 32-bit word per entry (spsp_downsample.hip).  Entry i of
// [0, n_keys) is kept iff (d_value[i] & need) == need and h_min <= (d_value[i] & 0x7fffffff) <= h_max (k_ds_flag_band); the kept keys
// of (d_mn, d_lo, d_hi) -- the caller's arrays already moved to the first entry -- go to (out_mn, out_lo, out_hi) through
// ds_compact_launch, W the carved area of (n_keys + kDsTile - 1) / kDsTile tiles and n_bounds offsets.  h_rel: the n_bounds offsets
// relative to the first entry; h_off_out receives the survivors in front of each.  Both are the CALLER's host arrays, read and
// written by queued copies: they live until the caller's wait.  Queued on the context's stream: no host wait
int ds_flag_compact_launch(spsp_ctx* ctx, const DsWork& W, bool has_hi, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint32_t* d_value,
                           uint32_t n_keys, uint32_t h_min, uint32_t h_max, uint32_t need, const uint64_t* h_rel, uint32_t n_bounds, uint32_t* out_mn,
                           uint64_t* out_lo, uint64_t* out_hi, uint64_t* total_host, uint64_t* h_off_out);
// the sorted distinct keys of n sketch payloads on the device, sketches back to back: the decoder's arrays, or the downsampling
// pass's (spsp_decode.hip).  ds_threshold: null = the keys as the files hold them; else only the keys whose minimizer passes that
// selection threshold, brought down on the device behind the decoder.  card[i] = the keys of sketch i that are left
struct DecodedKeys {
    uint32_t k = 0, m = 0;
    const uint32_t* mn = nullptr;
    const uint64_t *lo = nullptr, *hi = nullptr;                   // hi: null unless k > 32
    std::vector<uint64_t> sk_off;
};
int decode_keys_impl(spsp_ctx* ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n, const int* extra_has, const uint32_t* extra_mn,
                     const uint64_t* ds_threshold, DecodedKeys* keys, uint64_t* card);
// decode_keys_impl + all-vs-all + copy back: the device half of spsp_compare_files (spsp_decode.hip)
// (inter: n x n, zero on entry; *mirrored = every written cell (i, j > i) was also stored at (j, i))
// (cells_out, for 1024 <= n <= 65535: the non-zero cells i << 48 | j << 32 | count, every pair once, INSTEAD of the matrix: inter may be null)
int compare_payloads_impl(spsp_ctx* ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n, const int* extra_has,
                          const uint32_t* extra_mn, uint32_t n_query, const uint64_t* ds_threshold, uint32_t* k_out, uint32_t* m_out, uint32_t* inter,
                          uint64_t* card, bool* mirrored = nullptr, std::vector<uint64_t>* cells_out = nullptr);
// spsp_gather.hip: greedy gather of the first n_query sketches against the others over concatenated sorted key arrays; rows ordered by
// (query, rank).  gather_payloads_impl: decode_keys_impl + gather; card = the key counts the gather saw
int gather_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off,
                       uint32_t n, uint32_t nq, uint64_t min_keys, uint32_t max_rounds, std::vector<spsp_gather_row>* rows);
int gather_payloads_impl(spsp_ctx* ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n, uint32_t n_query, uint64_t min_keys,
                         uint32_t max_rounds, const uint64_t* ds_threshold, uint32_t* k_out, uint32_t* m_out, uint64_t* card,
                         std::vector<spsp_gather_row>* rows);
// spsp_cluster.hip: single-linkage clusters of the sketches 0 .. n-1 from the packed cells of their pair matrix (on the device, only
// read); cluster_payloads_impl: decode_keys_impl + the all-vs-all as cells + the cluster pass: the cells stay on the device;
// card = the key counts the comparison saw
int cluster_cells_impl(spsp_ctx* ctx, const uint64_t* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, int metric, uint32_t num,
                       uint32_t den, spsp_cluster_row* rows, uint64_t* n_clusters, uint64_t* n_edges);
int cluster_check_args(uint32_t n, int metric, uint32_t num, uint32_t den);
int cluster_payloads_impl(spsp_ctx* ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n, int metric, uint32_t num, uint32_t den,
                          const uint64_t* ds_threshold, uint32_t* k_out, uint32_t* m_out, uint64_t* card, std::vector<spsp_cluster_row>* rows,
                          uint64_t* n_clusters, uint64_t* n_edges);
// spsp_representatives.hip: greedy representatives of the sketches 0 .. n-1 from the packed cells (on the device, only read);
// h_weight: null = the key counts
int representatives_cells_impl(spsp_ctx* ctx, const uint64_t* d_cells, uint64_t n_cells, const uint64_t* h_card, const uint64_t* h_weight, uint32_t n,
                               int metric, uint32_t num, uint32_t den, spsp_cluster_row* rows, uint64_t* n_clusters, uint64_t* n_edges, uint32_t* n_rounds);
// spsp_tree.hip: the single-linkage tree (the maximum spanning forest in the order of include/spsp.h) of the sketches 0 .. n-1 from
// the packed cells (on the device, only read); num == 0 is a floor.  tree_rows_host (spsp_host.cpp): the forest's cell words, in
// any order -> the rows in the rule's order, with their sizes
int tree_check_args(uint32_t n, int metric, uint32_t num, uint32_t den);
int tree_cells_impl(spsp_ctx* ctx, const uint64_t* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, int metric, uint32_t num, uint32_t den,
                    spsp_tree_row* rows, uint64_t* n_rows, uint64_t* n_edges, uint32_t* n_rounds);
int tree_rows_host(const uint64_t* forest, uint64_t n_forest, const uint64_t* card, uint32_t n, int metric, spsp_tree_row* rows);
// spsp_neighbours.hip: each row sketch's best `top` partners at or above num / den from the packed cells (on the device, only read)
int neighbours_check_args(uint32_t n, uint32_t n_query, int metric, uint32_t num, uint32_t den, uint32_t top);
int neighbours_cells_impl(spsp_ctx* ctx, const uint64_t* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, uint32_t n_query, int metric,
                          uint32_t num, uint32_t den, uint32_t top, spsp_neighbour_row* rows, uint64_t cap, uint64_t* n_rows, uint32_t* passing,
                          uint64_t* n_pairs);
// spsp_prevalence.hip: per row sketch the keys by class of holder count and the sum of the counts, the spectrum of the references'
// union, h of every key occurrence (context-owned, on the device) -- over concatenated sorted key arrays, n_query == 0: all versus all
int prevalence_check_args(uint32_t n, uint32_t n_query, uint32_t num, uint32_t den);
// the argument front of a pass over concatenated sorted key arrays (prevalence, select, accumulation, groups), in this order: the
// context not switched to unordered keys ("<who_reads> sorted sketches: ..."), k in 1..63, offsets that do not decrease, an extent
// of 0xfffffff0 at the most (SPSP_ERR_OVERFLOW), no NULL key array where there are keys.  Touches nothing on the device
struct KeysShape { bool has_hi; uint64_t first, extent, all_keys; };
int sorted_keys_front(spsp_ctx* ctx, const char* who_reads, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi,
                      const uint64_t* h_sk_off, uint32_t n, KeysShape* shape);
// slots of a key table for `entries` entries, as a power of two: half as many again as the entries (every one may be a key of its
// own); SPSP_DEBUG_PREVALENCE_TABLE=min: the smallest that holds them, so that probe sequences wrap and chains are long
uint32_t pv_table_log2cap(uint64_t entries);
// the table fill the prevalence pass and the selection share: the sketch offsets uploaded (ctx->pv_off), the table cleared
// (ctx->pv_table), k_pv_count over the reference entries, k_pv_read over every entry -> ctx->pv_hold[e] = h of entry e.  claim: bit 31
// of pv_hold[e] is set as well iff entry e is the one that claimed its key's slot (exactly one occurrence of every distinct reference
// key; h <= 65535 leaves the bit free).  d_words: two u32 on the device the caller has cleared on the stream (keys out of order | a
// probe sequence that went round the table).  The caller has checked the arguments and the offsets.  Queued: no host wait
int prevalence_fill_table(spsp_ctx* ctx, bool has_hi, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off,
                          uint32_t n, uint32_t nq, bool claim, uint32_t* d_words);
// spsp_select.hip: the keys whose holder count lies in [h_min, h_max] as sketches again -- each: every row sketch's, order kept;
// merged: the distinct keys of the references' union, sorted, as ONE sketch -- in context-owned arrays
int keys_select_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n,
                     uint32_t nq, uint32_t h_min, uint32_t h_max, bool merged, uint32_t** out_mn, uint64_t** out_lo, uint64_t** out_hi, uint64_t* sk_off_out);
int prevalence_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off,
                           uint32_t n, uint32_t n_query, uint32_t num, uint32_t den, spsp_prevalence_row* rows, uint64_t* spectrum, uint32_t** d_holders);
// spsp_accumulation.hip: pan and core curves over orders of the sketches.  The pass kernel's geometry, which
// spsp_accumulation_plan_host (spsp_host.cpp) turns into the orders per pass and the window of ranks for a given n
constexpr uint32_t kAcPassThreads = 512;                   // 8 waves: one workgroup per CU once the rank tables fill its LDS
constexpr uint32_t kAcLdsBytes = 160 * 1024;               // what one workgroup may take on gfx950
constexpr uint32_t kAcBitmapBits = 8192;                   // per wave: the ranks one mex pass of a long list marks
constexpr uint32_t kAcMaxGroup = 8;                        // orders per pass at the most (their minima sit in registers)
constexpr uint32_t kAcCut = 64;                            // a list of more holders than this is queued for a whole wave (<= 64: the lane's mex mask); measured, DESIGN 6o
int accumulation_check_args(uint32_t n, uint32_t n_orders);
int accumulation_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off,
                             uint32_t n, const uint32_t* orders, uint32_t n_orders, spsp_accumulation_row* rows, uint64_t* pan, uint64_t* core);
// the key-major form of a collection, which the accumulation and the classification's index share (spsp_accumulation.hip): the
// table fill with claimers (prevalence_fill_table, all versus all), k_ac_prep, the two scans and k_ac_scatter, queued on the
// context's stream without a host wait.  words: the flag words (keys out of order | a probe sequence that went round or a list
// place out of range | the long lists queued); key_no[i]: the number of entry (first + i)'s key where that entry claimed the slot
// (the scan's value in front of it otherwise), key_no[E] = D, the distinct keys; key_start[0 .. D]; list: the holders' sketch
// numbers, list behind list; long_keys: the numbers of the keys with more than `cut` holders.  Behind it the table's counters are
// zero: a slot's low half still names the claimer.  The caller has been through sorted_keys_front and has at least one key
struct KeyMajor { uint32_t* words; const uint32_t* key_no; const uint32_t* key_start; const uint16_t* list; const uint32_t* long_keys; uint32_t entries; };
int key_major_build(spsp_ctx* ctx, bool has_hi, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n,
                    uint32_t cut, KeyMajor* out);
// spsp_classify.hip: the records of a batch against an index.  What routes a record (spsp_classify_plan_host, spsp_host.cpp):
constexpr uint32_t kCfThreads = 256;                       // probe, route, small form: 4 waves
constexpr uint32_t kCfSmallWork = 1024;                    // holders one wave of the small form sorts in LDS: a record of more work goes to a workgroup
constexpr uint32_t kCfLargeThreads = 512;                  // the large form: 8 waves per record
constexpr uint32_t kCfLargeFixedLds = 8 * 64 * 8 + 64;     // ... its LDS beside the counters: the waves' kept matches and the passing count
constexpr uint32_t kCfLdsRefs = (kAcLdsBytes - 8192) / 4;  // 38 912: up to this many references the large form's counters stay in LDS
constexpr uint32_t kCfListCut = 32;                        // the large form: a list of more holders than this is walked by the whole wave
constexpr uint32_t kCfMaxTop = 64, kCfMaxDen = 1000000;
int classify_check_args(uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den);
int classify_index_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n_ref);
int classify_device_impl(spsp_ctx* ctx, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, const uint64_t* h_rec_off, uint32_t n_rec,
                         uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den, spsp_classify_record* records, spsp_classify_hit* hits);
// the records path the record file drivers share (spsp_classify.hip): a FASTA / FASTQ text ingested and scanned once on a side
// context, a second context of ctx's device; the records' keys extracted there in batches of at most 65 535 records and handed to
// the pass's on_batch, whose work is queued on ctx (spsp_wait_stream orders the two contexts around every batch: the keys of a
// batch are read before the next extraction overwrites them).  Three plain types carry a run: RecordsAsk, what the caller asked;
// RecordPass, what differs between classify, taxonomy and depth; RecordsOut, what the road leaves behind for the driver
struct RecordBatch { uint32_t first_record, n_records; const uint32_t* mn; const uint64_t *lo, *hi; const uint64_t* key_off; };   // key_off: host, n_records + 1
// what the caller asked of a record file driver: filled in by the entry, read by everything below it.  mode: what is written
// beside the pass's CSVs -- nothing, the records a word names (extract), every record to the file of its bin (split) -- or in
// their place, the records cut into windows (windows).  what: the word of extract and split, the call word of windows.
// mates_path: null, or the second file of a paired run (records_paths[0] is the first then).  Depth and profile fill in the
// paths, rate, precision, out_prefix and chatter
enum RecordsMode { kRmPlain = 0, kRmExtract, kRmSplit, kRmWindows };
struct RecordsAsk {
    const char* const* records_paths = nullptr;
    uint32_t n_records_paths = 0;
    const char* mates_path = nullptr;
    RecordsMode mode = kRmPlain;
    const char* what = nullptr;
    int gz = 1;
    uint64_t window = 0;
    int precision = 6;
    const char* out_prefix = nullptr;
    int chatter = 0;
    double rate = 0;
    // a windowed run: stray runs of up to `smooth` windows are absorbed; segments_what: null, or the word that selects the segments
    // written as <out_prefix>_segments.fa (".gz" appended when gz), those of at least max(1, segments_min) bases
    uint32_t smooth = 0;
    const char* segments_what = nullptr;
    uint64_t segments_min = 1;
    // ... raw: the segments' raw intervals are made (one lift on the side context) and written as <out_prefix>_segments.bed
    int raw = 0;
};
// an entry's ask: records_path is the address of the entry's own argument, which outlives the call
inline RecordsAsk records_ask(const char* const* records_path, const char* mates_path, RecordsMode mode, const char* what, int gz, uint64_t window, int precision,
                              const char* out_prefix, int chatter, double rate) {
    RecordsAsk ask;
    ask.records_paths = records_path; ask.n_records_paths = 1; ask.mates_path = mates_path;
    ask.mode = mode; ask.what = what; ask.gz = gz; ask.window = window;
    ask.precision = precision; ask.out_prefix = out_prefix; ask.chatter = chatter; ask.rate = rate;
    return ask;
}
// what a pass is to the road and to the driver's tails; classify, taxonomy and depth (which serves profile) implement it.
// prelude: in front of the load (taxonomy: the lineage file, and extract's node against the tree).  on_index: once, behind the
// index.  on_records: once per file (or pair of files), behind the scan, with the records' base offsets
// (n_rec + 1; a pair: the mates' summed).  on_batch: a batch's keys, queued on ctx.  on_close: behind the last file, in front of
// the side contexts' end.  keep_flags / bins: the pass's rows -> keep[n] of extract's word / bin[n] and n_bins of split's or
// windows' word.  window_addends: window w's keys, hit keys and support.  bin_names (n_bins - 1) and last_name: for the manifest
// and the windowed CSVs.  write_rows: the pass's two CSVs, made and written in the pass's own order.  say_rows: its one
// chatter line.  A pass that has no rows to extract from (depth) keeps the refusals, which no entry reaches
struct FilesRun;
struct RecordPass {
    virtual ~RecordPass() {}
    virtual int prelude(const RecordsAsk&) { return SPSP_OK; }
    virtual int on_index() { return SPSP_OK; }
    virtual int on_records(uint32_t, const uint64_t*) { return SPSP_OK; }
    virtual int on_batch(const RecordBatch&) { return SPSP_OK; }
    virtual int on_close() { return SPSP_OK; }
    virtual int keep_flags(const char*, uint32_t, uint8_t*) { return no_rows(); }
    virtual int bins(const char*, uint32_t, uint32_t*, uint32_t*) { return no_rows(); }
    virtual void window_addends(size_t, uint32_t*, uint32_t*, uint32_t*) {}
    virtual const char* const* bin_names() { return nullptr; }
    virtual const char* last_name() { return ""; }
    virtual int write_rows(FilesRun&, const RecordsAsk&, const std::vector<std::string>&, double) { return SPSP_OK; }
    virtual void say_rows(FilesRun&, const RecordsAsk&) {}
    virtual size_t n_rows() { return 0; }
    static int no_rows() { set_error("this pass has no per-record rows to extract from"); return SPSP_ERR_ARG; }
};
// what a record file driver writes beside its CSVs when it is asked to (spsp_extract.hip, spsp_split.hip): one text's cut, on its
// side context.  The road asks the pass once per file (or pair of files) for keep[] or for bin[] and n_bins, behind the last
// batch and with the text still in the side context's buffer, and hands the plain vector to on_text (the extraction: the kept
// bytes to `out`) or split_text (every bin's slice to `out`, which bin_off cuts) of each run.  write: <out_prefix>_extract.fa or
// .fq (by the text's kind), gzip level 1 with ".gz" appended when gz, and with chatter the line of what was kept.  tag: "" for a
// records file alone; "_1" and "_2" for the two mates of the paired form, whose files are <out_prefix>_extract_1.* and _2.*
struct ExtractRun {
    const char* what = nullptr;
    const char* tag = "";
    int gz = 1;
    bool fastq = false;
    uint64_t n_rec = 0, n_kept = 0;
    std::vector<uint8_t> out;
    uint32_t n_bins = 0;
    std::vector<uint64_t> bin_off, bin_records;
    uint64_t bins_written = 0;
    int on_text(spsp_ctx* side, const uint8_t* d_text, uint64_t n_text, uint32_t n_rec, const uint8_t* keep);
    int split_text(spsp_ctx* side, const uint8_t* d_text, uint64_t n_text, uint32_t n_rec, const uint32_t* bin, uint32_t n_bins);
    int write(spsp_ctx* ctx, const char* out_prefix, int chatter);
};
// the windows run of a record file driver (spsp_windows.hip): the width; what the road leaves behind for the driver (first_win over
// the file's real records and their offsets, beside the windows the passes saw as records)
struct WindowsRun {
    uint64_t window = 0;
    std::vector<uint32_t> first_win;
    std::vector<uint64_t> rec_off;
    std::vector<spsp_segment_row> segments;
    std::vector<spsp_mosaic_row> mosaic;
    // the REAL records' cleaned bases on the side context, which TextSide::open replaces by the windows' for the scan: the ingest's
    // own buffer, which nothing behind the ingest writes, in the form `packed` says
    const uint8_t* d_bases = nullptr;
    uint64_t n_bases = 0;
    bool packed = false;
    // what the tail behind the last batch leaves for the driver: the three texts (made before any file is written), the windows
    // the smoothing changed, the segments selected and their bases
    uint32_t k = 0, n_bins = 0;
    std::string seg_csv, mos_csv;
    std::vector<uint8_t> fasta;
    bool want_fasta = false;
    uint64_t n_changed = 0, n_written = 0, bases_written = 0;
    // raw coordinates: the raw text on the side context (the ingest's upload, which nothing behind it writes: DESIGN 6zc); per
    // segment its raw interval (0, 0 for a segment without bases), the BED text, the segments lifted and the sequence characters
    // by which the raw intervals exceed the kept ones
    const uint8_t* d_text = nullptr;
    uint64_t n_text = 0;
    bool want_bed = false;
    std::vector<uint64_t> raw_begin, raw_end;
    std::string bed;
    uint64_t n_lifted = 0, raw_excess = 0;
};
// what the road leaves behind for the driver and the entry.  names: the records' names as the host reads them from the header
// lines (a pair: the mates' common names) -- then a text with another number of header lines than the device finds records is
// SPSP_ERR_FORMAT; want_names == false (depth: many files, no rows): no names, no header count.  t1: run.end().  extract: the
// one run, or the two mates'.  windows: behind the ingest and in front of the scan every record is cut into windows on the side
// context, and the scan, the seams, the key extraction, on_records and on_batch then see the WINDOWS as records; the header
// count is still held against the real records
struct RecordsOut {
    bool want_names = true;
    std::vector<std::string> names;
    double t1 = 0;
    ExtractRun extract[2];
    WindowsRun windows;
    uint64_t n_kept(const RecordsAsk& ask) const { return ask.mode == kRmSplit ? extract[0].bins_written : extract[0].n_kept; }
    uint64_t bytes_out() const { return extract[0].out.size() + extract[1].out.size(); }
};
// spsp_split.hip: the files and the manifest of a split run (mates: null, or the second mate's run; bin_names (n_bins - 1) and
// last_name: the pass's); spsp_host.cpp: a bin's file name
int split_write(spsp_ctx* ctx, ExtractRun* run, ExtractRun* mates, const char* const* bin_names, const char* last_name, const char* out_prefix, int chatter);
std::string split_file_name(const char* prefix, uint32_t b, uint32_t n_bins, const char* last_name, const char* tag, const char* suffix);
// what needs no device (spsp_host.cpp).  record_names_host: the records' names as the host reads them from the text, the first
// whitespace-delimited word of every header line -- FASTA: the lines that begin with '>'; FASTQ: every fourth line up to the
// content's end, which begins with '@'.  records_batch_bounds: 0, 65 535, 131 070, ..., n_rec -- batch b = records [bounds[b],
// bounds[b + 1]).  write_bytes: a file as it is, or gzip level 1 (the caller has appended ".gz")
void record_names_host(const uint8_t* text, uint64_t n, bool fastq, std::vector<std::string>* names);
std::vector<uint32_t> records_batch_bounds(uint32_t n_rec);
int write_bytes(const char* path, const uint8_t* data, uint64_t len, int gz);
// spsp_depth.hip: how many records hold each key of the index, and the per-reference statistics over those counts
constexpr uint32_t kDpThreads = 256;                       // every depth kernel: 4 waves
constexpr uint32_t kDpBins = 4096;                         // bins of one LDS histogram of k_dp_reduce: the last holds every count at or above kDpBins - 1
constexpr uint32_t kDpLongKeys = 65536;                    // a reference of more entries than this is reduced by segments, a workgroup each, and a merge
constexpr uint32_t kDpSegKeys = 16384;                     // ... of this many entries
int depth_begin_impl(spsp_ctx* ctx);
int depth_add_impl(spsp_ctx* ctx, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, uint64_t first, uint64_t n_keys);
int depth_read_impl(spsp_ctx* ctx, uint32_t min_count, spsp_depth_row* rows, spsp_depth_totals* totals, const uint32_t** d_entry_count);
// the two halves of a read's launches, for the profile as well (the context holds counters and its index has entries; no wait).
// depth_launch_entry: dp_entry = c per index entry, and the word d_found (64 bits, cleared here) = the index keys found at min_count.
// depth_launch_reduce: the rows of all references from dp_entry and a class byte per entry in the place of `unique` -> d_rows
int depth_launch_entry(spsp_ctx* ctx, uint32_t min_count, unsigned long long** d_found);
int depth_launch_reduce(spsp_ctx* ctx, const uint8_t* d_class, uint32_t min_count, spsp_depth_row* d_rows);
// spsp_depth_files behind its argument checks; with `profile` one spsp_profile_device call behind the read and
// <out_prefix>_profile.csv.gz beside the depth file
struct ProfileAsk { uint32_t min_keys, max_rounds; std::vector<spsp_profile_row> rows; spsp_profile_totals totals; };
int depth_files_impl(spsp_ctx* ctx, const char* const* paths, uint32_t n_ref, const char* const* reads_paths, uint32_t n_reads, uint32_t min_count, int precision,
                     const char* out_prefix, int chatter, double rate, std::vector<spsp_depth_row>* rows, spsp_depth_totals* totals, ProfileAsk* profile);
// spsp_profile.hip: the greedy rounds over the index's holder lists on the counters of the depth pass
constexpr uint32_t kPfPickThreads = 1024;                  // k_pf_pick: one workgroup
constexpr uint32_t kPfThreads = 256;                       // start and walk: 4 waves
constexpr uint32_t kPfListCut = kCfListCut;                // the walk: a list of more holders than this is walked by the whole wave
constexpr uint32_t kPfBatchFirst = 32, kPfBatchMax = 128;  // rounds queued per host wait: 32, 64, 128, 128, ...
int profile_impl(spsp_ctx* ctx, uint32_t min_count, uint32_t min_keys, uint32_t max_rounds, spsp_profile_row* rows, uint64_t* n_rows, spsp_profile_totals* totals,
                 const uint8_t** d_entry_assigned);
// spsp_taxonomy.hip: the records of a batch assigned to the lowest common ancestor of their keys.  What routes a record
// (spsp_taxonomy_plan_host, spsp_host.cpp):
constexpr uint32_t kTxThreads = 256;                       // key nodes, route, wave form: 4 waves
constexpr uint32_t kTxSmallHits = 1024;                    // hit keys one wave of the wave form sorts in its 4 KiB of LDS: a record of more goes to a workgroup
constexpr uint32_t kTxLargeThreads = 512;                  // the workgroup form: 8 waves per record
constexpr uint32_t kTxLargeFixedLds = 1024;                // ... its LDS beside the counters: the reductions' words and the way up
constexpr uint32_t kTxLdsNodes = (kAcLdsBytes - 8192) / 4; // 38 912: up to this many nodes the workgroup form's counters stay in LDS
constexpr uint32_t kTxListCut = kCfListCut;                // the key nodes: a list of more holders than this is folded by the whole wave
constexpr uint32_t kTxMaxNodes = 1048576, kTxMaxDepth = 32;
constexpr size_t kTxRowsBytes = (size_t)256 << 20;         // the workgroup form's rows in device memory, all of them: the grid is sized to fit
// What the two record calls share on the host (spsp_classify.hip; DESIGN "What the record passes share").
// refuse_no_index: the text of a call that finds no index in the context, under the pass's name.  record_keys_check: the key arrays
// of n_keys record keys against the index -- a NULL array, kmer_hi against the index's k -- which the depth pass's add has as well.
// record_call_front: what spsp_classify_device and spsp_taxonomy_device refuse behind their own threshold checks, in this order:
// the record count, decreasing offsets, the key count, no index, (needs_taxonomy) no taxonomy, and the two of record_keys_check;
// *all_keys: the keys of all records.  Every pass clears its outputs in front of it
int refuse_no_index(const char* pass);
int record_keys_check(const spsp_ctx* ctx, const char* pass, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, uint64_t n_keys);
int record_call_front(const spsp_ctx* ctx, const char* pass, bool needs_taxonomy, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi,
                      const uint64_t* h_rec_off, uint32_t n_rec, uint64_t* all_keys);
// one record call's device arrays, in the context's cf_ buffers: the record offsets, kn per record key, work and hit keys per record,
// the kRqWords words with the two queues behind them, and a row of row_bytes per record (16: classify, 32: taxonomy); g_route, g_small:
// the grids of the route kernel and of a wave form of kRecordWaves waves per workgroup.  reserve, then upload (the offsets) and
// clear (work, hit keys, words, rows) on the stream; read_back: the copies of the flag word and of the rows as 32-bit words, queued
// behind the last launch; wait: the call's one wait and the clock's spans; *fitted: no record overflowed the form it was routed to
constexpr uint32_t kRecordWaves = 4;
struct RecordWork {
    uint64_t* off; uint32_t* kn; unsigned long long* work; uint32_t *hit, *words, *q_small, *q_large; uint4* rec;
    uint32_t n_rec, g_route, g_small; uint64_t all_keys; size_t row_bytes;
    int reserve(spsp_ctx* ctx, uint32_t n_rec, uint64_t all_keys, size_t row_bytes);
    int upload(spsp_ctx* ctx, const uint64_t* h_rec_off);
    int clear(spsp_ctx* ctx);
    int read_back(spsp_ctx* ctx, std::vector<uint32_t>* rows);
    int wait(spsp_ctx* ctx, RecordClock& clock, bool* fitted);
};
// classify's probe pass, launched for another caller (spsp_classify.hip): kn[i] = the key number + 1 of record key i (0: nobody
// holds it), work[r] and hit[r] added up per record.  d_off: the record offsets on the device.  The caller has cleared work and hit
int classify_probe_launch(spsp_ctx* ctx, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, const uint64_t* d_off, uint32_t n_rec,
                          uint64_t all_keys, uint32_t* d_kn, unsigned long long* d_work, uint32_t* d_hit);
// the road of the record file drivers (spsp_classify.hip): run.load(ask.rate), the k == m refusal in the pass's words (what_is:
// "classification is", "depth is"), one record rate, the decoding and the index, pass.on_index behind it, then every records
// file read and sent through its batches on ONE second context (spsp_wait_stream(side, ctx) in front of every file: the last
// file's keys have been read) -- or, with ask.mates_path, records_paths[0] and it on two side contexts, the union of the two
// mates' keys per pair (spsp_union.hip) being what on_batch gets -- pass.on_close where all of that went well, the wait for
// ctx's stream and the side contexts' end; out->t1 = run.end()
int records_files_road(FilesRun& run, const char* what_is, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out);
// the one driver body behind classify and taxonomy (spsp_classify.hip): the runs' tags from the ask, the road (windows mode: its
// tail behind the last batch makes the texts, windows_tail), then windows_files or the pass's write_rows and, where asked, the
// extraction's or the split's files; the pass's chatter line and the common rate's
int record_files_run(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out);
// the front of the ten file entries.  record_files_check_args (spsp_host.cpp), in this order: NULL arguments (lineages_path with
// taxonomy, mates_path with paired, the word with windows), the reference count, the pass's thresholds, the word that belongs to
// the mode, the windows' width.  record_files_entry (spsp_classify.hip): those, hipSetDevice, the pass's prelude, record_files_run
struct RecordFront { spsp_ctx* ctx; const char* const* index_paths; const char* lineages_path; bool taxonomy, paired; uint32_t n_ref, top, min_keys, num, den; };
int record_files_check_args(const RecordFront& front, const RecordsAsk& ask);
int record_files_entry(const RecordFront& front, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out);
// several row arrays given out as give_rows gives one; where a later one fails, every array already given is freed and every
// pointer is null again.  An `out` that is null is passed over
struct RowsGift { void** out; const void* rows; size_t bytes; };
int give_rows_all(const RowsGift* gifts, size_t n);
int taxonomy_check_args(uint32_t min_keys, uint32_t num, uint32_t den);
int taxonomy_index_impl(spsp_ctx* ctx, const uint32_t* parent, uint32_t T, const uint32_t* ref_node, uint32_t n_ref, const uint32_t** key_nodes_out);
int taxonomy_device_impl(spsp_ctx* ctx, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, const uint64_t* h_rec_off, uint32_t n_rec,
                         uint32_t min_keys, uint32_t num, uint32_t den, spsp_taxonomy_record* records);
// spsp_extract.hip: the records of a text and the kept ones written out again (the rule: include/spsp.h).  What the kernels cut at
// (spsp_extract_plan_host, spsp_host.cpp):
constexpr uint32_t kExTile = 4096;                         // bytes of the text per workgroup of the starts pass (the ingest's tile)
constexpr uint32_t kExStretch = 16384;                     // bytes of the output one workgroup of the copy owns
constexpr uint32_t kExThreads = 256, kExRecsPerLane = 8, kExRecTile = kExThreads * kExRecsPerLane;   // every kernel: 4 waves; records per workgroup of the run table's passes
constexpr uint32_t kExStores = kExStretch / (kExThreads * 16);   // rounds of 16-byte stores a workgroup of the copy makes
// the words of one call on the device (64 bits each), ctx->ex_words.  The split (spsp_split.hip) uses them as the extraction does
enum ExWord {
    kExFastq = 0,   // k_ex_tail: 1 when the text is FASTQ
    kExLimit,       // ... where the content ends (FASTA: n)
    kExEnd,         // ... where the last record ends: begin[n_rec]
    kExUnits,       // the first scan's total: FASTA the starts behind byte 0, FASTQ the content's newlines (+ two words of the scan's)
    kExRecs = 6,    // k_ex_starts: the records
    kExBad,         // bit 0: a FASTQ content whose lines are not a multiple of four; bit 1: a pair of begin[] out of order or range;
                    // bit 2 (the split): more runs than the host counted from the bins
    kExSrc,         // the second scan's totals: the source bytes kept,
    kExRunsKept,    // ... the runs (low half) and the records kept (high half)
    kExNl,          // k_ex_rec_write: 1 when the last kept range gets its newline
    kExBlank,       // k_ex_tail: 1 when something follows the blank tail's first newline (the ingest's blank_tail): a content of
    kExEndEmpty,    // ... 4r + 3 lines then has an empty quality line, which ends here (behind the tail's second newline, or at n)
    kSpOut,         // the split's third scan's total: the output's bytes (+ one word of the scan's)
    kSpNlAt = 15,   // the split: the output byte that is the appended newline, or ~0
    kExWords = 16
};
struct ExSum;   // (spsp_device.h)
// the launches of the starts, for the extraction and the split (spsp_extract.hip).  ex_front: the text's alignment and its tiles.
// ex_count_launch: the tail, the tiles' sums and their scan -- everything that does not need n_rec -- with the call's words cleared
// in front.  ex_starts_launch: begin[0 .. cap] in ctx->ex_begin.  ex_scan_launch: out[i] = the sums of in[0 .. i), totals[0] = all a,
// totals[1] = all b | all c << 32, by one workgroup.  ex_refuse_lines: the refusal of a FASTQ content of `lines` lines.  No host wait
int ex_front(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t* n_tiles);
int ex_count_launch(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t n_tiles);
int ex_starts_launch(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t n_tiles, uint32_t cap);
int ex_scan_launch(spsp_ctx* ctx, const ExSum* d_in, uint64_t n_items, ExSum* d_out, unsigned long long* d_totals);
int ex_refuse_lines(uint64_t lines);
// begin[0 .. n_rec] in a context-owned buffer, with one host wait (for n_rec); *fastq (may be null): what the text is
int records_extents_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t** d_begin, uint32_t* n_rec, bool* fastq);
// the kept records back to back in a context-owned buffer, with one host wait (for n_out).  d_begin == null: the starts are made
// here, for n_rec records -- a text that holds another number is SPSP_ERR_ARG behind the wait, nothing having left the buffers
int records_extract_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_begin, uint32_t n_rec, const uint8_t* h_keep,
                         uint8_t** d_out, uint64_t* n_out, uint64_t* n_kept, bool* fastq);
// spsp_build.hip: the stable LSD radix sort of (64-bit key, 32-bit value) pairs by the keys' low `bits` bits, eight bits a pass
// (k_rs_hist, launch_scan_u32, k_rs_scatter per pass; tiles of kRsTile pairs; the histograms in ctx->bl_hist).  The result is in
// (*keys_io, *vals_io): the buffers swap with every pass.  bits == 0 launches nothing.  Queued on the context's stream: no host wait
constexpr uint32_t kRsThreads = 256, kRsPer = 8, kRsTile = kRsThreads * kRsPer;
int radix_sort_pairs(spsp_ctx* ctx, uint64_t** keys_io, uint32_t** vals_io, uint64_t* keys_tmp, uint32_t* vals_tmp, uint32_t n, uint32_t bits);
// spsp_split.hip: every record of a text written to the slice of its bin (the rule: include/spsp.h, "split").  What the kernels cut
// at is the extraction's (kExStretch, kExRecTile) and the sort's (kRsTile): spsp_split_plan_host, spsp_host.cpp
constexpr uint32_t kSpMaxBins = 1u << 24;
// the bins' slices back to back in the context's output buffer (the extraction's: a split and an extraction on one context
// overwrite each other's output), with one host wait.  d_begin == null: the starts are made here, for n_rec records
int records_split_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_begin, uint32_t n_rec, const uint32_t* h_bin, uint32_t n_bins,
                       uint8_t** d_out, uint64_t* n_out, uint64_t* h_bin_off, uint64_t* h_bin_records, bool* fastq);
// spsp_union.hip: per record the union of two sorted key lists (the rule: include/spsp.h, "paired records").  What the kernels cut
// at (spsp_union_plan_host, spsp_host.cpp):
constexpr uint32_t kUnThreads = 256;                       // every union kernel: 4 waves, a lane per key
constexpr uint32_t kUnTile = 256;                          // entries of B per count of the scan: one workgroup's, four ballot words
// the arrays are the context's (valid until its next union call); h_off: n_rec + 1, from 0.  One host wait
int records_union_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* a_mn, const uint64_t* a_lo, const uint64_t* a_hi, const uint64_t* h_a_off, const uint32_t* b_mn,
                       const uint64_t* b_lo, const uint64_t* b_hi, const uint64_t* h_b_off, uint32_t n_rec, uint32_t** out_mn, uint64_t** out_lo, uint64_t** out_hi,
                       uint64_t* h_off);
// spsp_windows.hip: every record cut into overlapping windows (the rule: include/spsp.h, "windows").  What the kernels cut at
// (spsp_windows_plan_host, spsp_host.cpp):
constexpr uint32_t kWnThreads = 256, kWnRecsPerLane = 8, kWnRecTile = kWnThreads * kWnRecsPerLane;   // every kernel: 4 waves; records per workgroup of the counting pass
constexpr uint32_t kWnStretchBytes = 16384;                // bytes of the output one workgroup of the copy owns, in either form
constexpr uint32_t kWnStretch = kWnStretchBytes;           // ... in bases of the ASCII form
constexpr uint32_t kWnStretchPacked = kWnStretchBytes * 4; // ... and of the packed form: whole dwords, whole 16-byte stores
constexpr uint32_t kWnStores = kWnStretchBytes / (kWnThreads * 16);   // rounds of 16-byte stores a workgroup of the copy makes
constexpr uint32_t kWnHalo = 256;                          // zero bytes behind the output's last stretch: what a scan may read
constexpr uint64_t kWnMaxWindows = 0xfffffff0ull, kWnMaxWidth = 0x7fffffffull;
// a record of L bases at width W and step S = W - (k - 1): its windows, and the bases of all of them together
__host__ __device__ inline uint64_t wn_count(uint64_t L, uint32_t k, uint64_t S) { return L < k ? 1ull : (L - k + S) / S; }   // ((L - k + 1) + S - 1) / S >= 1
__host__ __device__ inline uint64_t wn_bases(uint64_t L, uint64_t n_win, uint32_t k) { return L + (n_win - 1) * (uint64_t)(k - 1); }
// the windows of a text's records in the context's buffers, with one host wait (for the counts).  h_first_win: n_rec + 1
int records_windows_impl(spsp_ctx* ctx, const uint8_t* d_bases, uint64_t n_bases, const uint64_t* d_rec_off, uint32_t n_rec, uint32_t k, uint64_t window, bool packed,
                         uint8_t** d_out, uint64_t* n_out, uint64_t** d_win_off, uint32_t* h_first_win, uint64_t* n_windows);
// spsp_segments.hip: chosen segments written as FASTA from the cleaned bases (the rule: include/spsp.h, "segments as sequence").
// What the kernel cuts at (spsp_segments_plan_host, spsp_host.cpp):
constexpr uint32_t kSgLine = 80;                           // bases of a line (SPSP_SEGMENTS_LINE); a full line is kSgLine + 1 bytes
constexpr uint32_t kSgThreads = 256;                       // k_sg_write: 4 waves
constexpr uint32_t kSgStretch = 16384;                     // bytes of the text one workgroup owns: the extraction's schedule
constexpr uint32_t kSgStores = kSgStretch / (kSgThreads * 16);   // rounds of 16-byte stores a workgroup makes
constexpr uint32_t kSgLdsSegs = 512;                       // segments of a stretch whose table entries are kept in LDS (more: read from memory)
// the text in the context's buffer, queued on its stream: one upload, one launch, no host wait
int segments_write_impl(spsp_ctx* ctx, const uint8_t* d_bases, uint64_t n_bases, bool packed, const uint64_t* h_src, const uint64_t* h_len, const uint8_t* h_headers,
                        const uint64_t* h_hdr_off, uint64_t n_seg, uint8_t** d_out, uint64_t* n_out);
// the tail of a windowed run behind its last batch, with the side context still alive: the calls smoothed, segments and mosaic, the
// two CSV texts, where ask.raw is set the segments' ends through ONE records_lift_impl on `side` (its own wait) and the BED text,
// and where a word asks for it the selection, the headers, the write on `side` (ordered behind ctx by the caller)
// and the copy back, with one wait.  Nothing is written to disk here: windows_files does that, every text being made
int windows_tail(spsp_ctx* side, WindowsRun* run, const RecordsAsk& ask, uint32_t k, std::vector<uint32_t>& call, const std::vector<uint32_t>& keys,
                 const std::vector<uint32_t>& hit_keys, std::vector<uint32_t>& support, uint32_t n_bins, const std::vector<std::string>& names,
                 const char* const* call_names, const char* last_name);
int windows_files(spsp_ctx* ctx, WindowsRun* run, const RecordsAsk& ask, double t_csv);
// spsp_lift.hip: kept-base indices lifted to positions among the sequence characters of the raw text (the rule: include/spsp.h,
// "raw coordinates").  What the kernels cut at (spsp_lift_plan_host, spsp_host.cpp): the ingest's tile and chunk
constexpr uint32_t kLfTile = 4096, kLfChunk = 16, kLfThreads = kLfTile / kLfChunk;
// raw[q] (and rec[q], raw_length[r] where asked) in the caller's host arrays, with one host wait.  *n_rec: in, where raw_length
// is given, the records it has room for; out, the records of the text
int records_lift_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t n_bases, const uint64_t* h_base, uint64_t n_q, uint64_t* raw, uint32_t* rec,
                      uint64_t* raw_length, uint32_t* n_rec);
// the selection of an ask held before any file is read (spsp_host.cpp); the header of one segment's FASTA record
int segments_ask_check(const RecordsAsk& ask, int taxonomy, uint32_t n_bins);
void segment_header(const spsp_segment_row& g, const char* name, const char* const* call_names, const char* last_name, uint32_t n_bins, std::string* s);
// spsp_groups.hip: per-group core, exclusive and marker keys of a partitioned collection; with want_markers the marker keys of the
// groups as n_groups sketches back to back in context-owned arrays
int groups_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n,
                       const uint32_t* h_group, uint32_t n_groups, uint32_t num, uint32_t den, uint32_t onum, uint32_t oden, spsp_group_row* rows,
                       spsp_group_member_row* members, bool want_markers, uint32_t** out_mn, uint64_t** out_lo, uint64_t** out_hi, uint64_t* marker_off);
// the front half of every file driver (spsp_host.cpp): the payloads of n sketch files, in file order, and what their headers say
struct LoadedSketches {
    std::vector<uint8_t*> data;                                    // into the context's read regions, or owned (own[i])
    std::vector<uint64_t> len;
    std::vector<uint8_t> own;
    uint32_t k = 0, m = 0;                                         // of the first header (0 until it has been read)
    std::vector<int> extra_has;                                    // the first-read chain (spsp_sketch_chain_host)
    std::vector<uint32_t> extra_mn;
    // a common sampling rate was asked for (rate_asked): the rate, its selection threshold, the sketches finer than it, and whether
    // there are any (ds_on: the device has something to bring down)
    bool rate_asked = false, ds_on = false;
    uint64_t ds_threshold = 0;
    double ds_rate = 0;
    uint32_t ds_brought = 0;
    double t0 = 0;                                                 // when the loading began
    const uint64_t* threshold() const { return ds_on ? &ds_threshold : nullptr; }   // what the *_payloads_impl take
    void release();                                                // frees the payloads it owns (the regions stay with the context)
    LoadedSketches() = default;
    LoadedSketches(const LoadedSketches&) = delete;
    LoadedSketches& operator=(const LoadedSketches&) = delete;
    ~LoadedSketches() { release(); }
};
// rate: SPSP_RATE_AS_IS = the headers' rates are ignored, as the reference does; SPSP_RATE_COARSEST or a rate = every header's rate
// is read and held against it (a coarser sketch is refused), and the device half is to bring the finer ones down
int load_sketch_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, double rate, LoadedSketches* L);
// what the file drivers' tails share (spsp_host.cpp).  files_loaded: the reference's first line (Comparator.cpp:56) and the
// loading booked to load_s; returns the time the device half starts at
double files_loaded(spsp_ctx* ctx, const LoadedSketches& L, uint32_t n, int chatter);
// text (taken over: freed here) -> <out_prefix><suffix> at gzip level 1; csv_s is booked from t_csv to here, csv_gzip_s from here on
int write_csv_gz(spsp_ctx* ctx, char* text, uint64_t len, const char* out_prefix, const char* suffix, double t_csv);
// the line that names the common rate, where one was asked for (not the reference's: behind its own lines)
void say_common_rate(const LoadedSketches& L, uint32_t n);
// spsp_select.hip: the rate a driver writes into the headers of the sketches it makes -- the common one where one was asked for, else
// the headers' own if they all stand for one selection threshold, else SPSP_ERR_ARG ("give a rate")
int sketches_out_rate(const LoadedSketches& L, const char* const* paths, uint32_t n, double* out_rate);
// selected keys on their way into sketch files.  fetch_keys (spsp_select.hip): `total` keys of device arrays copied to the host,
// with its own wait.  write_key_sketches (spsp_host.cpp): segment i = keys [off[i], off[i + 1]) -> a sketch file name_of(i)
// (spsp_sketch_from_keys_host, gzip level 9 as the sketcher writes); list_path: null, or where the names go, one per line
struct HostKeys { std::vector<uint32_t> mn; std::vector<uint64_t> lo, hi; };
int fetch_keys(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, uint64_t total, HostKeys* keys);
int write_key_sketches(uint32_t k, uint32_t m, double rate, const HostKeys& keys, const uint64_t* off, uint32_t n_out,
                       const std::function<std::string(uint32_t)>& name_of, const char* list_path);
// the opening and closing of a file driver behind a collection pass: load, the k == m refusal, the booking of a failed load or
// files_loaded, the decoding, and release + the booking of compare_s.  A driver calls the steps in ITS order (select and groups
// refuse k == m only behind a good load; select books and releases by itself, around its writing)
struct FilesRun {
    spsp_ctx* ctx;
    const char* const* paths;
    uint32_t n;
    int chatter;
    LoadedSketches L;
    std::vector<uint64_t> card;                                    // the key counts the pass saw
    DecodedKeys keys;
    double t0 = 0;                                                 // when the device half began
    FilesRun(spsp_ctx* c, const char* const* p, uint32_t n_, int chat) : ctx(c), paths(p), n(n_), chatter(chat), card(n_, 0) {}
    int load(double rate) { return load_sketch_files(ctx, paths, n, rate, &L); }
    // what_is: "clustering is", "neighbours are", ...; rc: the load's, returned where there is nothing to refuse
    int refuse_k_eq_m(int rc, const char* what_is) {
        if (!L.k || L.k != L.m) return rc;
        set_error("%s not defined for k == m sketches (k = m = %u)", what_is, L.k);
        return SPSP_ERR_ARG;
    }
    int begin(int rc) {
        if (rc) { ctx->stages.compare_s += now_s() - L.t0; return rc; }
        t0 = files_loaded(ctx, L, n, chatter);
        return SPSP_OK;
    }
    int decode() { return decode_keys_impl(ctx, L.data.data(), L.len.data(), n, nullptr, nullptr, L.threshold(), &keys, card.data()); }
    double end() {
        L.release();
        const double t1 = now_s();
        ctx->stages.compare_s += t1 - t0;
        return t1;
    }
};
// a driver's rows as the caller's array to spsp_free (one byte for no rows: never NULL on success)
template <class T> int give_rows(const std::vector<T>& rows, T** out) {
    const size_t bytes = rows.size() * sizeof(T);
    *out = (T*)malloc(bytes ? bytes : 1);
    if (!*out) { set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    if (bytes) memcpy(*out, rows.data(), bytes);
    return SPSP_OK;
}
int sketch_decode_device_impl(spsp_ctx* ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n,
                              const int* extra_has, const uint32_t* extra_mn, uint32_t* k_out, uint32_t* m_out, uint64_t* sk_off);
// ingest (spsp_ingest.hip)
// pack: the cleaned bases leave as 2-bit words (ctx->packed: 16 bases per dword, first base in bits 31:30, zero-filled tail
// + 256 readable bytes) instead of ASCII (ctx->bases); *d_bases then points at the words
// FASTQ: how the ingest reads a text that holds FASTQ (spsp_ingest.hip).  tile_info == nullptr: the whole text is one FASTQ
// file whose content -- the text less its trailing blank lines -- ends at content_end, and a malformed record is an
// SPSP_ERR_FORMAT of the call.  Otherwise one word per 4 KiB tile describes a batch of files (FASTA and FASTQ, each starting
// a tile) and bad[f] receives, per file, ~0 or (the first malformed record, numbered in the batch) << 8 | rule.
constexpr uint32_t kTiLim = 0x1FFFu;          // FASTQ: bytes of the tile that belong to the file's content (0..4096)
constexpr uint32_t kTiFastq = 1u << 13;
constexpr uint32_t kTiStart = 1u << 14;       // a file starts at the tile's first byte
constexpr uint32_t kTiBlankTail = 1u << 15;   // FASTQ: a blank line follows the file's last non-blank line
constexpr int kTiFileShift = 16;              // bits 16..23: the file's index in the batch
constexpr uint32_t kTiEnd = 1u << 24;         // FASTQ: the file's content ends inside the tile
enum { kFqBadHeader = 1, kFqBadSeparator = 2, kFqBadLength = 3, kFqTruncated = 4 };
struct FastqLayout {
    const uint32_t* tile_info = nullptr;      // host
    uint64_t content_end = 0;
    bool blank_tail = false;
    uint32_t n_files = 1;
    uint64_t* bad = nullptr;                  // host, n_files words
};
// the content end of a FASTQ text (behind its last byte that is neither '\n' nor '\r') and whether a blank line follows it
void fastq_tail(const uint8_t* text, uint64_t n, uint64_t* content_end, bool* blank_tail);
// One file of a batch, as the table builder needs it: its place in the slab (a multiple of the 4 KiB tile), whether it has a
// place at all, whether it failed behind the layout (its region is all newlines), its format and, for FASTQ, what fastq_tail says
struct BatchFile {
    uint64_t off = 0;
    bool laid = false, failed = false, fastq = false;
    uint64_t fq_end = 0;
    bool fq_blank = false;
};
// the tile words (kTi*) of a batch of `total` bytes: tinfo gets one word per tile; files are in slab order, bits 16..23 of a
// file's tiles hold its index in `files`
void batch_tile_table(const BatchFile* files, size_t n_files, uint64_t total, std::vector<uint32_t>* tinfo);
const char* fastq_rule_name(uint32_t rule);
int clean_device_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint8_t** d_bases, uint64_t* n_bases,
                      uint64_t** d_rec_off, uint32_t* n_rec, bool pack = false, const FastqLayout* fq = nullptr);
// does the dense pass chosen for these parameters read 2-bit input directly? (spsp_scan.hip)
bool scan_reads_packed(const spsp_params* p);
bool build_on_device(uint64_t places);    // the sketch builder on the device from 5 x 10^5 k-mer places on (SPSP_BUILD=device / host pins it)
// should the whole-file drivers let the ingest write 2-bit words for these parameters? (spsp_ingest.hip)
bool ingest_packs(const spsp_params* p);
int gather_superkmers_impl(spsp_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_rec_off, const spsp_superkmer* d_sk,
                           uint64_t n_sk, uint8_t** h_compact, uint32_t** h_off, bool packed = false);
// out[i] = sum(in[0..i)), out[n] = total (also stored to *total_host, pinned)
int launch_scan_u32(spsp_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, uint64_t n, uint64_t* total_host);
int sketch_stream_stats(const spsp_params* p, const uint64_t* rec_off, uint32_t n_rec, const spsp_superkmer* sk, uint64_t n_sk, spsp_sketch_stats* st);
void sketch_header_line(uint32_t k, uint32_t m, uint64_t selected_kmers, double rate, std::string& out);
// the sketch builder on the device (spsp_build.hip): the bodies of n_files sketches from the scan's stream; file_stats: per file
// actual_minimizer_number, seen_kmers_at_reconstruction, seen_superkmers_at_reconstruction, seen_max_superkmers_at_reconstruction
int sketch_build_device_impl(spsp_ctx* ctx, const spsp_params* p, const uint8_t* d_bases, bool packed, const uint64_t* d_rec_off, const spsp_superkmer* d_sk,
                             uint64_t n_sk, const uint32_t* h_file_sk, uint32_t n_files, std::vector<std::string>* bodies, std::vector<uint64_t>* file_stats);
// zstr-style inflate of a whole buffer: gzip / zlib members, or the bytes as they are (spsp_host.cpp)
int inflate_all_host(const uint8_t* in, size_t n, std::vector<uint8_t>& out);
// host sketch builder over per-super-k-mer base pointers (spsp_host.cpp)
// -a on the device (spsp_abund.hip): per k-mer occurrence of the gathered super-k-mers, bit 0 usable, bit 1 first of a dropped k-mer
int abundance_flags_impl(spsp_ctx* ctx, const spsp_params* p, const spsp_superkmer* d_sk, uint64_t n_sk, uint8_t** h_flags, uint64_t* n_occ_out,
                         const uint32_t* h_seg_sk = nullptr, uint32_t n_seg = 0);
// exchange slots of the key-partitioned split (wire format: spsp_compare.hip, sender; spsp_multi.hip, receiver)
constexpr uint32_t kSlotMagic = 0x4c535053u;   // "SPSL"
constexpr uint32_t kMaxParts = 64;
__host__ __device__ inline uint64_t slot_rec_off(uint32_t n) { return 16 + (uint64_t)((n + 1) & ~1u) * 4; }
__host__ __device__ inline uint32_t slot_words(uint32_t k) { return k > 32 ? 3u : 2u; }
__host__ __device__ inline uint64_t slot_bytes(uint32_t n, uint32_t cap, uint32_t k) {
    return slot_rec_off(n) + (uint64_t)cap * slot_words(k) * 8;
}
int partition_keys_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_min, const uint64_t* d_lo, const uint64_t* d_hi,
                        const uint64_t* h_sk_off, uint32_t n, uint32_t parts, uint32_t cap, uint8_t* d_slots);
int compare_slots_begin_impl(spsp_ctx* ctx, uint32_t k, const uint8_t* d_slots, uint32_t parts, uint32_t n, uint32_t cap,
                             uint32_t* d_inter, const uint8_t* h_headers = nullptr);
int slots_bad_record(spsp_ctx* ctx);
// sparse form of a pair matrix (spsp_multi.hip): non-zero cells (i < j) as i << 48 | j << 32 | count
int matrix_cells_impl(spsp_ctx* ctx, const uint32_t* d_inter, uint32_t n, uint32_t row_first, uint32_t row_limit, uint64_t* d_cells,
                      uint64_t cap, uint64_t* n_cells);
// queue a comparison with begin() and return its pair matrix as sparse cells: straight from the row sums where the form allows
// it (d_scratch then stays unwritten), else through the dense matrix in d_scratch (n x n uint32) and k_matrix_cells
int compare_cells_run(spsp_ctx* ctx, const std::function<int()>& begin, uint32_t n, uint32_t row_limit, uint32_t* d_scratch, uint64_t* d_cells,
                      uint64_t cap, uint64_t* n_cells, DevBuf* grow = nullptr);
// the all-vs-all of decoded keys as cells in ctx->m_cells (rows below row_limit): room for max(2^16, 32 n) cells first, and once
// more with the exact room where that was too little
int compare_keys_cells(spsp_ctx* ctx, const DecodedKeys& keys, uint32_t n, uint32_t row_limit, uint64_t* n_cells);
// decode + all-vs-all over several contexts (one per device, or several on one): the device half of spsp_compare_files_multi
// (ds_threshold as in decode_keys_impl: every context brings its own block down before the keys are dealt into exchange slots)
int compare_payloads_multi(spsp_ctx* const* ctxs, uint32_t n_ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n,
                           const int* extra_has, const uint32_t* extra_mn, uint32_t n_query, const uint64_t* ds_threshold, uint32_t* k_out,
                           uint32_t* m_out, uint32_t* inter, uint64_t* card, bool* mirrored = nullptr, std::vector<uint64_t>* cells_out = nullptr);
// spsp_bigkeys.hip: distinct keys of flagged segments through one table in HBM (queued, no host wait); segments sorted in place
int big_dedupe_launch(spsp_ctx* ctx, bool has_hi, const uint32_t* raw_mn, const uint64_t* raw_lo, const uint64_t* raw_hi,
                      const uint32_t* d_seg_first, const uint32_t* d_seg_cnt, const uint32_t* d_seg_big, uint32_t n_seg, uint64_t n_places,
                      const uint32_t* d_gate, uint32_t abundance, uint32_t* out_mn, uint64_t* out_lo, uint64_t* out_hi, uint32_t* d_distinct);
int big_sort_segments(spsp_ctx* ctx, bool has_hi, uint32_t* mn, uint64_t* lo, uint64_t* hi, uint32_t* t_mn, uint64_t* t_lo, uint64_t* t_hi,
                      const std::vector<std::pair<uint32_t, uint32_t>>& segs);
int sketch_build_core(const spsp_params* p, double rate, const uint64_t* rec_off, uint32_t n_rec, const spsp_superkmer* sk,
                      uint64_t n_sk, const uint8_t* bases, const uint8_t* compact, const uint32_t* compact_off,
                      uint8_t** payload, uint64_t* payload_len, spsp_sketch_stats* stats, const uint8_t* kmer_flags);
}  // namespace spsp
