/* spsp.h -- C-ABI of libspsp: the MI355X-native drop-in for SuperSampler's
 * data-parallel hot path (sketch scan + all-vs-all sketch comparison).
 *
 * The reference (TimRouze/supersampler) has no FFI seam of its own: its public
 * surface is two CLIs and three file formats.  This header is
 * the seam a maintainer would bind instead of calling the member functions
 * cited next to each entry point (paths relative to the reference tree).
 *
 * Conventions: plain pointers and sizes, no exceptions cross the boundary,
 * 0 = ok / negative = error (text from spsp_last_error(), thread-local).
 * Buffers returned through `**out` are owned by the library and released with
 * spsp_free().  A context is bound to
 * one HIP device + one stream and is not shared between threads: the CLIs use
 * one context (= one stream) per in-flight genome.
 *
 * Every entry point whose name does not end in _host runs on the GPU and
 * FAILS (SPSP_ERR_NO_DEVICE) when no gfx950 device is usable -- there is no
 * CPU fallback in this library.
 */
#ifndef SPSP_H
#define SPSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPSP_OK 0
#define SPSP_ERR_ARG (-1)
#define SPSP_ERR_NO_DEVICE (-2)
#define SPSP_ERR_HIP (-3)
#define SPSP_ERR_NOMEM (-4)
#define SPSP_ERR_IO (-5)
#define SPSP_ERR_FORMAT (-6)
#define SPSP_ERR_OVERFLOW (-7)

typedef struct spsp_ctx spsp_ctx;

/* Scan parameters: the state `Subsampler::Subsampler` derives from the command
 * line (SubSampler.h:63-88). k, m odd, m <= 15, m <= k <= 63. */
typedef struct spsp_params {
    uint32_t k;
    uint32_t m;
    uint64_t threshold; /* selection_threshold, from spsp_threshold_host() */
    uint32_t abundance; /* -a, used by the sketch builder only */
    uint32_t flags;     /* SPSP_SCAN_* */
} spsp_params;

#define SPSP_SCAN_DEFAULT 0u
#define SPSP_SCAN_DIRECT_HASH 1u /* force XXH64 at every position (no LDS pre-filter) */
#define SPSP_SCAN_LDS_FILTER 2u  /* force the 2^20-bit memoised LDS pre-filter (one lookup per position) */
#define SPSP_SCAN_PAIR_FILTER 4u /* force the 64 KiB pair table (one lookup per two positions, m >= 9) */
#define SPSP_SCAN_PACKED_INPUT 32u /* device forms only: d_bases holds 2-bit codes (spsp_pack_bases_device), not ASCII */
#define SPSP_SCAN_BLOOM_FILTER 16u /* force the blocked Bloom filter over canonical m-mers (m = 13 or 15) */
#define SPSP_SCAN_STATS 8u       /* spsp_sketch_text / spsp_sketch_file: also count EVERY super-k-mer of the input
                                    (total_superkmer_number of print_stat, SubSampler.cpp:430,452) -- an extra pass */

/* One selected super-k-mer == one call of Subsampler::handle_superkmer
 * (SubSampler.cpp:426,448): ref.substr(start,len) of record `rec`, its
 * minimizer (canonical 2-bit value) and whether that minimizer reads
 * reverse-complemented in the genome. Emitted in genome order. */
typedef struct spsp_superkmer {
    uint32_t rec;
    uint32_t minimizer;
    uint64_t start; /* offset inside the record */
    uint32_t len;
    uint32_t rev;
} spsp_superkmer;

/* One sketch as the comparator sees it after Comparator.cpp:186-260: the
 * DISTINCT canonical k-mers of every bucket, sorted by (minimizer, kmer_hi,
 * kmer_lo). kmer_hi may be NULL when k <= 32. */
typedef struct spsp_sketch_view {
    const uint32_t* minimizer;
    const uint64_t* kmer_lo;
    const uint64_t* kmer_hi;
    uint64_t n;
} spsp_sketch_view;

/* ------------------------------------------------------------ lifecycle -- */
/* how many gfx950 devices this process sees (devices 0 .. count - 1 are usable with spsp_create); 0 = none, see spsp_last_error */
int spsp_device_count(void);
int spsp_create(int device, void* hip_stream /* hipStream_t or NULL = own stream */, spsp_ctx** out);
void spsp_destroy(spsp_ctx* ctx);
const char* spsp_last_error(void);
const char* spsp_version(void);
void spsp_free(void* host_ptr);
/* CU partitioning (MI355X: 256 CUs in 8 XCDs).  spsp_stream_create_cus makes a HIP stream whose kernels may only
 * run on the `n_cu` logical compute units [first_cu, first_cu + n_cu) (hipExtStreamCreateWithCUMask; the mask's bits
 * are dealt round-robin over the XCDs -- measured, tools/exp/exp_cumask.hip -- so a range of 8j bits is j CUs of every
 * XCD).  A pipeline gives the bandwidth-bound dense pass most of the chip and the latency-bound kernels (sparse
 * stages, comparison) a few CUs of their own: they then overlap without slowing each other down, which they do when
 * they share CUs (a dense workgroup next to a comparison workgroup runs at half speed and the dense grid, a static
 * partition, waits for it).  Take n_cu in multiples of 32: a CU count that is not the same in every shader engine
 * (4 per XCD) makes the dispatcher double workgroups up on some CUs (dense pass 0.10 -> 0.15 ms with 240 CUs).
 * spsp_set_cu_count tells a context how many CUs its stream owns (grid sizing; 0 = all) and how many dense-pass
 * workgroups to put on each: 1 (the default) leaves half of every CU's wave slots and LDS to other streams' kernels,
 * 2 is for a stream that has its CUs to itself. */
int spsp_stream_create_cus(int device, uint32_t first_cu, uint32_t n_cu, void** hip_stream);
int spsp_stream_destroy(int device, void* hip_stream);
int spsp_set_cu_count(spsp_ctx* ctx, uint32_t n_cu, uint32_t dense_blocks_per_cu);
/* copy `bytes` from a device buffer returned by this library to host memory, on the context's stream, and wait */
int spsp_copy_to_host(spsp_ctx* ctx, void* dst, const void* d_src, uint64_t bytes);

/* ------------------------------------------------------------ measurement -- */
/* HIP-event timing of the two dominant kernels and of the whole pipelines, on
 * the context's stream (bench.py's `roofline` numbers come from here). */
typedef struct spsp_timing {
    double dense_ms;       /* k_dense: hash + threshold over every m-mer position */
    uint64_t dense_launches;
    double scan_ms;        /* whole spsp_scan_device pipeline */
    uint64_t scan_calls;
    double accumulate_ms;  /* k_accumulate: colour-matrix row sums */
    uint64_t accumulate_launches;
    double compare_ms;     /* whole spsp_compare_device pipeline */
    uint64_t compare_calls;
    double scatter_ms;     /* k_parts_scatter: keys dealt into hash classes (partition form of the comparison) */
    uint64_t scatter_launches;
    double group_ms;       /* k_parts_group: per-class LDS dictionary -> sketch lists */
    uint64_t group_launches;
} spsp_timing;
/* `kinds` = OR of SPSP_TIME_* (0 = off).  Every bracketed region costs two event records on the stream, i.e. two
 * packets the following kernels queue behind (~5 us each on an otherwise idle queue): enable what you read.
 * The scan / compare pipeline brackets close behind the FIRST attempt a begin call queues: the re-run of a call
 * whose buffers overflowed (or whose key classes did) is not inside the bracket. */
#define SPSP_TIME_DENSE 1
#define SPSP_TIME_SCAN 2
#define SPSP_TIME_ACCUMULATE 4
#define SPSP_TIME_COMPARE 8
#define SPSP_TIME_PARTS 16 /* scatter + group kernels */
#define SPSP_TIME_ALL 31
int spsp_timing_enable(spsp_ctx* ctx, int kinds);
/* bracket only every `every`-th region of each kind (1 = all): the two event packets of a bracket cost a pipelined
 * stream ~4 us each (bench.py: 8.6 us of a 0.123 ms step with every dense pass bracketed) */
int spsp_timing_sample(spsp_ctx* ctx, uint32_t every);
/* synchronises the stream, returns the totals since the previous read and resets them */
int spsp_timing_read(spsp_ctx* ctx, spsp_timing* out);

/* HBM calibration for the roofline's denominator ("calibrate with a device copy kernel on the box and use
 * the measured figure"; the reference has no counterpart -- its only timer is Comparator.cpp:499-509): a streaming copy
 * and a streaming read of two freshly allocated buffers of `bytes` each (take >= 1 GiB: the 256 MiB Infinity Cache must
 * not serve them), `reps` launches each behind two warm-up launches, timed with HIP events on the context's stream and
 * on the CUs that stream owns.  copy_GBps counts bytes read + bytes written. */
typedef struct spsp_hbm_rates {
    double copy_GBps, copy_ms;   /* per launch */
    double read_GBps, read_ms;
    uint64_t bytes;
    uint32_t reps, n_cu;
} spsp_hbm_rates;
int spsp_measure_hbm_device(spsp_ctx* ctx, uint64_t bytes, uint32_t reps, spsp_hbm_rates* out);

/* ------------------------------------------------------------- path A ---- */
/* Subsampler::compute_threshold + ctor selection (SubSampler.cpp:622-631,
 * SubSampler.h:79-83). Host long double, as the reference. */
uint64_t spsp_threshold_host(uint32_t k, uint32_t m, double sampling_rate);

/* Replaces the scan loop SubSampler.cpp:357-455 with regular_minimizer_pos
 * :81-169 and unrevhash :64-67. `bases` = cleaned upper-case ASCII records
 * back to back (what getLineFasta returns, utils.cpp:706-718); rec_off has
 * n_rec+1 entries. Output: the handle_superkmer argument stream. */
int spsp_scan(spsp_ctx* ctx, const spsp_params* p, const uint8_t* bases, const uint64_t* rec_off,
              uint32_t n_rec, spsp_superkmer** out, uint64_t* n_out);

/* Same with everything resident in HBM (16-byte aligned d_bases). The result
 * stays on the device in a buffer OWNED BY THE CONTEXT (*d_out: n_out records,
 * valid until the next scan call on this context; do not free). The whole
 * pipeline is queued on the context's stream and the call returns after the one
 * host synchronisation that reads back *n_out. */
int spsp_scan_device(spsp_ctx* ctx, const spsp_params* p, const void* d_bases, uint64_t n_bases,
                     const void* d_rec_off, uint32_t n_rec, void** d_out, uint64_t* n_out);

/* 2-bit input (0.25 B per k-mer hashed).  spsp_pack_bases_device turns `n_bases` cleaned ASCII bases on the
 * device into the packed form -- 16 bases per little-endian 32-bit word, first base in bits 31:30, A=0 C=1 T=2 G=3, the
 * last word zero-filled and 256 readable bytes behind it -- in a buffer the context owns (valid until its next pack call).
 * A scan whose spsp_params.flags carry SPSP_SCAN_PACKED_INPUT takes that buffer as d_bases (n_bases stays the number of
 * BASES; record offsets are base offsets as ever).  The pair-table and the blocked-Bloom dense passes (m >= 9 at coarse
 * sampling; m = 13 / 15 at fine sampling: BASELINE configs[1] and configs[4]) read it directly: a quarter of the traffic, no
 * packing arithmetic; the other variants unpack it into an ASCII copy first.  Same stream out. */
int spsp_pack_bases_device(spsp_ctx* ctx, const void* d_bases, uint64_t n_bases, void** d_packed);

/* The same call split at its host synchronisation, for callers that pipeline several streams (one context
 * per stream): _begin queues the whole scan on the context's stream and returns at once; _end waits for it,
 * and re-runs the affected stages in the rare call whose hit / super-k-mer buffers overflowed.  One scan
 * may be pending per context.  d_bases / d_rec_off must stay valid until _end returns. */
int spsp_scan_device_begin(spsp_ctx* ctx, const spsp_params* p, const void* d_bases, uint64_t n_bases,
                           const void* d_rec_off, uint32_t n_rec);
int spsp_scan_device_end(spsp_ctx* ctx, void** d_out, uint64_t* n_out);
/* Optional second stream for the scan's sparse stages: everything behind the dense pass (hit compaction, cluster
 * replay) is queued on `hip_stream` (NULL = a stream the context creates itself; pass tail = 0 to switch back),
 * ordered behind the dense pass by an event.  Several contexts created on ONE stream then run their dense passes
 * back to back in that stream's order while each context's sparse stages overlap the next dense pass. */
int spsp_scan_tail_stream(spsp_ctx* ctx, int tail, void* hip_stream);
/* Stream ordering between two contexts of one device: work queued on `waiter` after this call starts only
 * once the dense pass of `scanner`'s most recently queued scan has finished (the dense pass fills every CU;
 * latency-bound work of another stream overlaps best with the sparse stages behind it). */
int spsp_wait_dense(spsp_ctx* waiter, spsp_ctx* scanner);
/* ... only once everything queued on `other` so far has finished. */
int spsp_wait_stream(spsp_ctx* waiter, spsp_ctx* other);

/* total_superkmer_number of Subsampler::print_stat (SubSampler.cpp:430,452,641): how many super-k-mers the scan
 * loop cuts over ALL k-mers of the input, selected or not -- including the cuts its position tracking makes
 * when one m-mer occurs twice in a window (`dump`, :391-398).  Not needed for the sketch: a separate pass. */
int spsp_count_superkmers_device(spsp_ctx* ctx, const spsp_params* p, const void* d_bases, uint64_t n_bases,
                                 const void* d_rec_off, uint32_t n_rec, uint64_t* total_superkmers);
/* What the last scan collected on the context (spsp_scan_device, spsp_scan_device_end and every call that scans through
 * them) and the last super-k-mer count did: both have two forms that give the same numbers, and a caller or a test that has
 * to know which one answered reads it here.  Read-only; nothing is launched or waited for.
 *   counts[0]  the form that gave the last collected scan's stream: 0 none yet, or an empty call; 1 the scan by segments
 *              (thresholds of 0.8 x 2^64 and more, -s 1); 2 the product scan (dense + sparse passes); 3 the product scan after
 *              the scan by segments counted and reported a chain that it did not finish (it left its tile's halo and the walk
 *              behind it was refused or ran out)
 *   counts[1]  the number of such unfinished chains that scan reported (0 unless counts[0] is 1 or 3)
 *   counts[2]  the form that gave the last spsp_count_superkmers_device total (also the SPSP_SCAN_STATS pass of the sketch
 *              calls): 0 none yet, or a call without a k-mer; 1 the count by segments and its tail kernel; 2 the chunk kernels
 *              from the start; 3 the chunk kernels after the count by segments handed over (more chains left their halos than
 *              the tail kernel has lanes)
 *   counts[3]  the chains that left their tile's halo in that count (0 when counts[2] is 0 or 2) */
int spsp_stats_counts(spsp_ctx* ctx, uint32_t* counts /* 4 */);

/* Dense stage only (hash + threshold + hit bitmap), for the roofline
 * measurement: returns the number of m-mers with hash <= threshold. */
int spsp_scan_hits_device(spsp_ctx* ctx, const spsp_params* p, const void* d_bases, uint64_t n_bases,
                          uint64_t* n_hits);

/* ------------------------------------------------------------- path B ---- */
/* Replaces Comparator::count_intersection / skip_bucket / compute_scores
 * (Comparator.cpp:97-287): inter is n*n, entry [a*n+b] for a<b =
 * sum over buckets |A_a,b ∩ A_b,b| (zero elsewhere); card[i] = nb_kmer_seen_infile[i].
 * Query mode (n_query < n, the sketches of the -q file first): only rows a < n_query are computed --
 * the rows print_jaccard / print_containment emit (Comparator.cpp:374,423); other rows stay zero. */
int spsp_compare(spsp_ctx* ctx, const spsp_sketch_view* sk, uint32_t n, uint32_t n_query,
                 uint32_t* inter, uint64_t* card);

/* Device-resident form over concatenated key arrays (sketch i owns entries
 * [d_sk_off[i], d_sk_off[i+1]) ). Only the rows row_first, row_first + row_stride, ... below n_query
 * are computed (the multi-GPU split of SURVEY.md 8e: every rank holds all sketches after the
 * all-gather and owns a share of the rows -- a block: row_first = its first row, row_stride = 1,
 * n_query = the end of the block; or strided: row_first = rank, row_stride = ranks, n_query = n).
 * A call that owns a part of the rows builds its dictionary from the owned sketches' keys; the other
 * sketches' keys are read once and kept only where an owned sketch may hold them too, and sketches
 * in front of row_first are not read at all (a row counts the sketches behind it). d_inter is a
 * dense n*n uint32 matrix; cells (i, j > i) of owned rows are overwritten, everything else is left
 * untouched. The work is queued on the context's stream: results are complete once that stream has
 * drained. */
int spsp_compare_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo,
                        const void* d_kmer_hi /* NULL if k<=32 */, const uint64_t* h_sk_off,
                        uint32_t n, uint32_t n_query /* = n for all-vs-all */, uint32_t row_first,
                        uint32_t row_stride, void* d_inter);

/* ----------------------------------- multi-GPU exchange ---- */
/* The reference is single-process; its all-vs-all merge (Comparator.cpp:97-287) has no sharded form to mirror.
 * Key-partitioned split: equal (minimizer, k-mer) keys hash to the same rank, every rank counts its own hash
 * class for ALL pairs, and inter = the sum of the partial matrices (sparse: spsp_matrix_cells_device).  Each rank sends each of
 * its keys exactly once (all-to-all) -- O(own keys) per rank, against O(all keys) for an all-gather.
 *
 * Sender: scatter this rank's n sketches (concatenated key arrays as in spsp_compare_device) into `parts`
 * fixed-size slots, slot p for rank p, at d_slots + p * spsp_slot_bytes(n, slot_cap, k) (8-byte aligned).
 * Slot layout: u32 magic, u32 n, u32 n_keys, u32 words; u32 cnt[n] (padded to even); slot_cap records of
 * `words` u64 (kmer_lo, [kmer_hi if k > 32], minimizer | local sketch << 32), grouped by sketch, original
 * order kept.  A slot with more than slot_cap keys keeps the first slot_cap and records the true n_keys: the
 * receiver reports SPSP_ERR_OVERFLOW and the caller partitions again with a larger slot_cap. Asynchronous
 * on the context's stream. */
uint64_t spsp_slot_bytes(uint32_t n, uint32_t slot_cap, uint32_t k);
int spsp_partition_keys_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo,
                               const void* d_kmer_hi /* NULL if k<=32 */, const uint64_t* h_sk_off, uint32_t n,
                               uint32_t parts, uint32_t slot_cap, void* d_slots);
/* Receiver: d_slots holds `parts` slots, slot s as sent by rank s (same n, slot_cap, k everywhere). Global
 * sketch id = s * n + local id; d_inter is the dense (parts*n)^2 uint32 partial matrix: cells (i, j > i)
 * are overwritten with this rank's share of |K_i ∩ K_j|, everything else is left untouched.  The slot headers
 * (geometry, keys per sketch) are read on the host first -- a malformed slot is SPSP_ERR_FORMAT, one that
 * overflowed at the sender SPSP_ERR_OVERFLOW, before any kernel reads it -- then the records are unpacked into
 * flat key arrays and go through the same partition-form comparison as spsp_compare_device, every row owned. */
int spsp_compare_slots_device(spsp_ctx* ctx, uint32_t k, const void* d_slots, uint32_t parts, uint32_t n,
                              uint32_t slot_cap, void* d_inter);

/* spsp_compare_device / spsp_compare_slots_device split at their host synchronisation (see
 * spsp_scan_device_begin): _begin queues the dictionary build, colour matrix and row sums and returns;
 * spsp_compare_end waits, checks the input / collision flags and, after a fingerprint collision, rebuilds
 * with a new seed.  One comparison may be pending per context; h_sk_off is copied before _begin returns,
 * the device arrays must stay valid until spsp_compare_end returns. */
int spsp_compare_device_begin(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo,
                              const void* d_kmer_hi, const uint64_t* h_sk_off, uint32_t n, uint32_t n_query,
                              uint32_t row_first, uint32_t row_stride, void* d_inter);
int spsp_compare_slots_device_begin(spsp_ctx* ctx, uint32_t k, const void* d_slots, uint32_t parts, uint32_t n,
                                    uint32_t slot_cap, void* d_inter);
int spsp_compare_end(spsp_ctx* ctx);

/* --------------------------------------------- host side of the two CLIs -- */
/* getLineFasta + clean_dna (utils.cpp:675-718) over an already gunzipped
 * buffer: records back to back + n_rec+1 offsets. */
int spsp_fasta_clean_host(const char* text, uint64_t n, uint8_t** bases, uint64_t** rec_off,
                          uint32_t* n_rec);

/* The same two functions on the GPU ("next" row N1): raw gunzipped FASTA text resident in HBM (16-byte
 * aligned) -> cleaned records + offsets in context-owned device buffers, ready for spsp_scan_device. */
int spsp_fasta_clean_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, void** d_bases, uint64_t* n_bases,
                            void** d_rec_off, uint32_t* n_rec);

/* ... with the cleaned bases written as 2-bit words straight away (utils.cpp:675-718 compacted AND packed in one pass:
 * N1 of SURVEY.md 8f): *d_packed is the layout spsp_pack_bases_device makes -- 16 bases per little-endian dword, first
 * base in bits 31:30, zero tail, 256 readable bytes behind -- in a context-owned buffer, ready for a scan with
 * SPSP_SCAN_PACKED_INPUT; n_bases and the record offsets count BASES as ever.  spsp_sketch_text / spsp_sketch_file(s) use
 * it whenever the dense pass of their parameters reads packed input (the pair-table pass: the default configuration). */
int spsp_fasta_clean_packed_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, void** d_packed, uint64_t* n_bases,
                                   void** d_rec_off, uint32_t* n_rec);

/* FASTQ read sets.  A text whose first byte is '@' is FASTQ: records of exactly four lines -- '@' header, sequence, '+'
 * separator, quality as long as the sequence (lengths counted without a trailing '\r'; the last record may lack its
 * newline; blank lines may follow the last record).  Each read is one record; its bases are the sequence line cleaned as
 * clean_dna cleans FASTA.  Sketching FASTQ text T is sketching the FASTA text that holds ">" + header[1:] + "\n" + seq +
 * "\n" per record.  Wrapped (multi-line) FASTQ is not read.  The two calls below mirror spsp_fasta_clean_device and
 * spsp_fasta_clean_packed_device (same arguments, output layout and ownership); a malformed record is SPSP_ERR_FORMAT
 * and spsp_last_error() names its 0-based index and the rule it breaks.  spsp_sketch_text, spsp_sketch_file(s) and
 * spsp_sketch_files_multi tell the format from the first byte of each (gunzipped) text or file; in a batch a malformed
 * FASTQ file fails alone. */
int spsp_fastq_clean_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, void** d_bases, uint64_t* n_bases,
                            void** d_rec_off, uint32_t* n_rec);
int spsp_fastq_clean_packed_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, void** d_packed, uint64_t* n_bases,
                                   void** d_rec_off, uint32_t* n_rec);

/* The batch form of the ingest, as spsp_sketch_files runs it, callable on its own (the tests hold it to exact bytes).
 * slab: HOST bytes laid out as the file pipeline lays a batch out -- file 0 at offset 0, every file on a multiple of 4096,
 * a FASTA text that is empty or starts with neither '>' nor 0xFF with one '>' forced in front (counted in text_len), '\n' from
 * a file's end up to the next multiple of 4096 strictly behind it, where the next file starts; n_slab is where the last file's
 * fill ends.  SPSP_BATCH_FASTQ: the file is read as FASTQ.  SPSP_BATCH_FAILED: the file could not be read, its region holds
 * '\n' alone and it has no record.  Up to 256 files (more: SPSP_ERR_ARG).  Outputs as spsp_fasta_clean_device (packed != 0:
 * as spsp_fasta_clean_packed_device), the records of all files in order, and two caller-owned host arrays:
 * rec_base[n_slab / 4096], the ingest's record base per tile (at a file's first tile: 1 + the file's first record), and
 * bad[n_files]: ~0, or (the file's first malformed record, numbered in the batch) << 8 | rule (1 header, 2 separator, 3 length,
 * 4 truncated).  A malformed file keeps its records and fails no call. */
typedef struct spsp_batch_file {
    uint64_t off, text_len;
    uint32_t flags, reserved;
} spsp_batch_file;
#define SPSP_BATCH_FASTQ 1u
#define SPSP_BATCH_FAILED 2u
int spsp_ingest_batch(spsp_ctx* ctx, const void* slab, uint64_t n_slab, const spsp_batch_file* files, uint32_t n_files, int packed,
                      void** d_out, uint64_t* n_bases, void** d_rec_off, uint32_t* n_rec, uint32_t* rec_base, uint64_t* bad);

typedef struct spsp_sketch_stats {
    uint64_t read_kmer, selected_kmer_number, selected_superkmer_number, count_maximal_skmer;
    uint64_t seen_kmers_at_reconstruction, seen_superkmers_at_reconstruction;
    uint64_t seen_max_superkmers_at_reconstruction, actual_minimizer_number, nb_mmer_selected;
    uint64_t total_kmer_number, total_superkmer_number;   /* filled when SPSP_SCAN_STATS is set, else 0 */
} spsp_sketch_stats;

/* handle_superkmer + the emission half of parse_fasta_test
 * (SubSampler.cpp:243-302, 458-504, 512-620; strCompressor utils.cpp:48-68):
 * super-k-mer stream -> uncompressed sketch payload. `rate` is the -s value
 * after stof (SubSampler.cpp:699), printed into the header.  Buckets (minimizers) are
 * built one by one -- they never meet -- and, from 20 000 super-k-mers on, on up to
 * 8 (16 from 400 000 on) host threads of the call's own: same bytes out. */
int spsp_sketch_build_host(const spsp_params* p, double rate, const uint8_t* bases,
                           const uint64_t* rec_off, uint32_t n_rec, const spsp_superkmer* sk,
                           uint64_t n_sk, uint8_t** payload, uint64_t* payload_len,
                           spsp_sketch_stats* stats);

/* FASTA (or FASTQ: see above) text (host) -> sketch payload with ingest, scan and super-k-mer gather on the GPU: what
 * parse_fasta_test does between openFile and the gzip writer (SubSampler.cpp:306-504). */
int spsp_sketch_text(spsp_ctx* ctx, const spsp_params* p, double rate, const char* text, uint64_t n_text,
                     uint8_t** payload, uint64_t* payload_len, spsp_sketch_stats* stats);

/* The sketch builder on the device (spsp_build.hip) from host buffers, as spsp_scan is to spsp_scan_device: what
 * spsp_sketch_build_host computes, for n_files files at once, whatever SPSP_BUILD or the number of k-mer places say.  The
 * stream is as the scan writes it (`rec` counts over all files' records, `start` and `len` inside the record), file f's
 * super-k-mers are sk[file_sk[f] .. file_sk[f + 1]).  packed != 0: the bases are first brought into the 2-bit words the
 * ingest writes, and the builder reads those.  *payloads: every file's whole payload (header line with that file's selected
 * k-mer number, then its buckets), back to back, file f at payload_off[f] .. payload_off[f + 1]; spsp_free() it.  counters:
 * four per file -- actual_minimizer_number, seen_kmers_at_reconstruction, seen_superkmers_at_reconstruction,
 * seen_max_superkmers_at_reconstruction.  n_sk == 0: header lines only.
 * SPSP_ERR_ARG, before anything is launched and with nothing written: a NULL argument; parameters out of range; n_files == 0;
 * rec_off that does not start at 0 or decreases; file_sk that does not start at 0, decreases or does not end at n_sk; a
 * super-k-mer outside its record or shorter than k (spsp_sketch_build_host's message), with a minimizer >= 4^m, or with
 * rev > 1.  The minimizer is NOT checked to be the k-mers' minimum, nor to occur in them: a k-mer that does not hold it is
 * indexed with the place 255, as the reference's find() leaves it.  SPSP_ERR_OVERFLOW (the builder's own, passed through): more than 2^25 super-k-mers, 2^31 k-mer
 * places or 4 GiB of payloads in one call. */
int spsp_sketch_build_device(spsp_ctx* ctx, const spsp_params* p, double rate, const uint8_t* bases, const uint64_t* rec_off,
                             uint32_t n_rec, const spsp_superkmer* sk, uint64_t n_sk, const uint32_t* file_sk, uint32_t n_files,
                             int packed, uint8_t** payloads, uint64_t* payload_off, uint64_t* counters);

/* Header + bucket reader of the comparator (Comparator.cpp:23-37, 78-92,
 * 186-260; strDecompressor utils.cpp:71-111): payload -> sorted distinct
 * (minimizer, canonical k-mer) keys. Arrays are spsp_free()d one by one. */
int spsp_sketch_parse_host(const uint8_t* payload, uint64_t len, uint32_t* k, uint32_t* m,
                           uint32_t** minimizer, uint64_t** kmer_lo, uint64_t** kmer_hi, uint64_t* n);

/* From a scan straight to the comparator's keys, without the sketch file in between.  Genome g = records
 * [h_first_rec[g], h_first_rec[g + 1]) of ONE scan (d_bases / n_bases / d_rec_off / d_superkmers as given to and returned by
 * spsp_scan_device; SPSP_SCAN_PACKED_INPUT in p->flags when d_bases holds 2-bit words).  The result is what
 * spsp_sketch_parse_host would return for the sketch parse_fasta_test writes for that genome: handle_superkmer's
 * per-k-mer counts with their uint8 wrap and the -a rule (SubSampler.cpp:243-302, 587, 608), the emission / reader round
 * trip (:458-620, Comparator.cpp:186-260) and canonize composed -- the DISTINCT (minimizer, canonical k-mer) keys of every
 * genome, sorted, back to back in device arrays OWNED BY THE CONTEXT (the ones spsp_sketch_decode_device fills: valid
 * until the next decode / keys / spsp_compare call on it; *d_kmer_hi = NULL when k <= 32), sk_off with n_genomes + 1
 * offsets: ready for spsp_compare_device.  A genome of ANY size stays on the device, like the reference's unbounded
 * minimizer_map (SubSampler.h:62): up to 8192 selected k-mer occurrences (4096 with k > 32) a workgroup handles a genome in
 * its LDS; a larger one is flagged by that workgroup and taken by the global-memory stages queued behind it in the same
 * call (one open-addressing table in HBM with the same per-(k-mer, orientation) counts and uint8 rule; then, for the
 * sorted form, a merge sort of the genome's distinct keys where they finally lie, queued from _end).  There is no host
 * path.  _begin queues the work on the context's stream and returns; _end waits for it (an event behind its last
 * kernel).  The caller's device inputs (bases, record offsets, super-k-mers) are read by the work _begin queues and by
 * nothing else: they may be rewritten once that work has run -- spsp_scan_output_wait orders a scan's next write
 * behind it -- without waiting for _end.  One job may be pending per context.
 * flags: SPSP_KEYS_UNORDERED -- every genome's keys DISTINCT but in no particular order: an LDS table per genome instead of
 * the per-genome sort (a tenth of its time; up to 6144 k-mer places and 1024 super-k-mers per genome, 4096 / 512 with
 * k > 32, beyond that the same global-memory table, without the sort).  Such keys are for
 * comparisons on a context that has been told so (spsp_compare_keys_unordered): the comparison itself only needs a
 * sketch to hold a key once; the order is what lets it CHECK that on input it did not make. */
#define SPSP_KEYS_UNORDERED 1u
int spsp_sketch_keys_device(spsp_ctx* ctx, const spsp_params* p, const void* d_bases, uint64_t n_bases, const void* d_rec_off,
                            const void* d_superkmers, uint64_t n_superkmers, const uint32_t* h_first_rec, uint32_t n_genomes, uint32_t flags,
                            void** d_minimizer, void** d_kmer_lo, void** d_kmer_hi, uint64_t* sk_off);
int spsp_sketch_keys_device_begin(spsp_ctx* ctx, const spsp_params* p, const void* d_bases, uint64_t n_bases, const void* d_rec_off,
                                  const void* d_superkmers, uint64_t n_superkmers, const uint32_t* h_first_rec, uint32_t n_genomes, uint32_t flags);
/* on != 0: the device-form comparisons queued on this context from now on accept sketches whose keys are distinct but
 * unsorted (the caller vouches for "distinct": duplicates inside a sketch would be counted twice) */
int spsp_compare_keys_unordered(spsp_ctx* ctx, int on);
/* A context remembers what its last comparisons looked like (the input came in a good row order, most records had lists,
 * parts spilled, the filter's pass rate) and queues the next one accordingly -- scheduling only, results never depend on it.
 * This forgets all of it: for timing or profiling comparisons of different collections on one context.
 * SPSP_DEBUG_SPILL_TRACE=1 prints the form every comparison took on stderr. */
int spsp_compare_forget(spsp_ctx* ctx);
int spsp_sketch_keys_device_end(spsp_ctx* ctx, void** d_minimizer, void** d_kmer_lo, void** d_kmer_hi, uint64_t* sk_off);
/* how many genomes of the extraction last collected on this context were beyond the per-genome LDS forms and went
 * through the table in HBM (a diagnostic for tests and benchmarks) */
uint32_t spsp_sketch_keys_big_genomes(spsp_ctx* ctx);

/* A scan's output buffer belongs to its context and is rewritten by that context's next scan.  A caller that pipelines --
 * queues scan t + 1 on `scanner` while `reader`'s key extraction of scan t's output (spsp_sketch_keys_device_begin) may
 * still be running on another stream -- calls this in between: the stage of the next scan that writes the output (its
 * last) then starts only behind the reader's latest key extraction; the dense pass is not held up. */
int spsp_scan_output_wait(spsp_ctx* scanner, spsp_ctx* reader);

/* The same decode for MANY sketches at once on the GPU ("next" row N2): payloads[i] = gunzipped sketch i.  The
 * sorted distinct keys of all sketches end up back to back in device arrays OWNED BY THE CONTEXT (valid until the
 * next decode / spsp_compare call on it; *d_kmer_hi = NULL when k <= 32), ready for spsp_compare_device; sk_off gets
 * n + 1 offsets.  A sketch of any size is decoded on the device (beyond 8192 raw keys -- 4096 with k > 32 -- through a
 * table in HBM and a merge sort instead of the per-sketch LDS sort); only a sketch that is not laid out as the sketcher
 * writes it goes through spsp_sketch_parse_host internally: same keys. */
int spsp_sketch_decode_device(spsp_ctx* ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n,
                              uint32_t* k, uint32_t* m, void** d_minimizer, void** d_kmer_lo, void** d_kmer_hi,
                              uint64_t* sk_off);

/* The comparator's N-way merge reads every file's first minimizer into one shared buffer without an end-of-file
 * check (Comparator.cpp:294,316-319).  Call this for the sketches IN FILE ORDER with the same `read_buffer` (m bytes,
 * initialised to 'A'): it performs that read and, for a sketch without any bucket when k == m, returns the one
 * phantom key the reference then counts for it (has_key = 1).  spsp_compare_files does this itself. */
int spsp_sketch_chain_host(const uint8_t* payload, uint64_t len, uint32_t k, uint32_t m, char* read_buffer, int* has_key,
                           uint32_t* minimizer, uint64_t* kmer_lo, uint64_t* kmer_hi);

/* print_jaccard / print_containment (Comparator.cpp:362-460), IEEE division.
 * names: n NUL-terminated strings. */
int spsp_csv_host(int jaccard, const char* const* names, uint32_t n, uint32_t n_query,
                  const uint32_t* inter, const uint64_t* card, int precision, double min_threshold,
                  char** text, uint64_t* len);

/* The same two printers from the SPARSE form of the pair matrix: `cells` = its non-zero entries as packed words
 * i << 48 | j << 32 | count (i < j < n <= 65535, every pair at most once, any order: what spsp_compare_cells_device
 * returns).  A comparison of thousands of sketches has ~10 non-zero partners per row; a row is then written as runs of
 * "0," between them and no n x n matrix is built or scanned.  Same bytes as spsp_csv_host on the dense matrix. */
int spsp_csv_cells_host(int jaccard, const char* const* names, uint32_t n, uint32_t n_query, const uint64_t* cells, uint64_t n_cells,
                        const uint64_t* card, int precision, double min_threshold, char** text, uint64_t* len);
/* The same matrix written straight to `gz_path` as the reference writes it (gzip, Comparator.cpp:363,413), without the text
 * ever existing: row blocks become gzip members on the host threads, a run of "0," cells is two literals and a few deflate
 * matches of distance 2, and the member's CRC-32 takes the run in 16 table steps (spsp_compare_files writes its two
 * 10^8-cell matrices this way).  gunzip gives exactly the bytes spsp_csv_cells_host returns. */
int spsp_csv_cells_gz_host(int jaccard, const char* const* names, uint32_t n, uint32_t n_query, const uint64_t* cells, uint64_t n_cells,
                           const uint64_t* card, int precision, double min_threshold, const char* gz_path);

/* sortCSV (sort_csv.cpp:26-111): rows and columns of a symmetric all-vs-all Jaccard CSV (gunzipped text) put into
 * the order of the original file of files.  Inputs the reference mishandles (name missing from the fof or listed
 * twice, short or unparsable rows, diagonal != 1) are rejected with SPSP_ERR_FORMAT. */
int spsp_sort_csv_host(const char* csv, uint64_t csv_len, const char* fof, uint64_t fof_len, char** text, uint64_t* len);

/* zstr-compatible I/O (include/zstr.hpp:136-209 autodetect, :392-407 gzip
 * writer): whole-file read with gzip/zlib/plain autodetection; gzip write. */
int spsp_read_file_host(const char* path, uint8_t** data, uint64_t* len);
int spsp_write_gz_host(const char* path, const uint8_t* data, uint64_t len, int level);

/* Whole-file drivers used by the CLIs (Subsampler::parse_fasta_test
 * SubSampler.cpp:306-510; Comparator::compare_sketches + printers
 * Comparator.cpp:39-74, 362-460). */
int spsp_sketch_file(spsp_ctx* ctx, const spsp_params* p, double rate, const char* fasta_path,
                     const char* out_path, spsp_sketch_stats* stats);
/* The file-of-files loop of the reference's main (`#pragma omp parallel num_threads(c)`, SubSampler.cpp:771-793) inside
 * the library: the n files are taken in list order, a few at a time; `threads` workers read (and gunzip) a batch's files
 * into one pinned buffer, the batch crosses PCIe in one copy and goes through ONE ingest, ONE scan and ONE gather on the
 * GPU (a GPU job per file is a chain of launches and host waits that costs ~0.35 ms however small the file), and the
 * workers then run the sketch builder, gzip and the write per file.  Up to four batches (at most one per worker) are in flight, each on a
 * context (HIP stream) of its own, so reading, the GPU and the builders overlap inside ONE process.  With -a > 1 the
 * k-mer occurrences of the whole batch are counted in one device pass, file by file (the file is part of the key).  A batch
 * with 5 x 10^5 selected k-mer occurrences or more (one metagenome file) has its sketches BUILT on the device as well
 * (handle_superkmer + the emission walk, spsp_build.hip; SPSP_BUILD=device / host pins the choice).  `cb` (may be
 * NULL) is called with phase 0 when file `index` is taken off the queue (inside the queue's lock: the calls come in
 * list order, like the reference's critical(fof) section that prints the name and appends to the output list; with ONE
 * worker right before the file's own phase-1 call, the way the reference's single thread alternates names and reports) and
 * with phase 1 when it is done (rc, its statistics, the error text when rc != 0; one call at a time, like critical(cout)).
 * A file that fails does not stop the others; the call then returns SPSP_ERR_IO.  `times` (may be NULL) receives the
 * stage seconds summed over the workers. */
typedef void (*spsp_file_callback)(void* user, uint32_t index, int phase, int rc, const spsp_sketch_stats* stats, const char* error);
int spsp_sketch_files(int device, const spsp_params* p, double rate, const char* const* fasta_paths, const char* const* out_paths,
                      uint32_t n, uint32_t threads, spsp_file_callback cb, void* user, struct spsp_stage_times* times);
/* The same over several GPUs of one node: the batches are dealt over the devices (slot j of the pipeline lives on
 * devices[j mod n_dev]; up to four batches in flight per device), everything else as above -- sketching shards by genome,
 * there is nothing to exchange.  A device may be named more than once. */
int spsp_sketch_files_multi(const int* devices, uint32_t n_dev, const spsp_params* p, double rate, const char* const* fasta_paths,
                            const char* const* out_paths, uint32_t n, uint32_t threads, spsp_file_callback cb, void* user,
                            struct spsp_stage_times* times);
/* spsp_sketch_files keeps its contexts, device buffers and pinned staging buffers for the next call on the same device
 * (setting them up costs more than sketching a hundred genomes).  This releases the idle ones (device < 0: of every
 * device); optional -- a process that simply exits never needs it. */
void spsp_sketch_files_release(int device);
/* Wall-clock seconds the two whole-file drivers have spent per stage on this context (end-to-end measurement:
 * bench.py's `end_to_end` object).  GPU stages include the host synchronisation that ends them. */
typedef struct spsp_stage_times {
    double read_s;     /* sketch: file read + gunzip (zstr autodetect)                      utils.cpp:357-364 */
    double ingest_s;   /* sketch: H2D copy + getLineFasta/clean_dna on the GPU               utils.cpp:675-718 */
    double scan_s;     /* sketch: the minimizer scan                                         SubSampler.cpp:357-455 */
    double gather_s;   /* sketch: selected super-k-mers' bases back to the host */
    double build_s;    /* sketch: handle_superkmer + emission on the host                    SubSampler.cpp:243-302,458-504 */
    double gzip_s;     /* sketch: gzip level 9 + write                                       SubSampler.cpp:326 */
    double load_s;     /* compare: read + gunzip + decode + sort of all sketches (host threads)  Comparator.cpp:186-260 */
    double compare_s;  /* compare: H2D + all-vs-all on the GPU + D2H                         Comparator.cpp:97-287 */
    double csv_s;      /* compare: both matrices formatted                                   Comparator.cpp:362-460 */
    double csv_gzip_s; /* compare: gzip level 1 + write */
    uint64_t sketch_files, compare_calls;
} spsp_stage_times;
int spsp_stage_times_read(spsp_ctx* ctx, spsp_stage_times* out, int reset);
int spsp_compare_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query,
                       int precision, double min_threshold, const char* out_prefix);
/* the same, printing the progress lines of the reference's comparator on stdout where it prints them
 * (Comparator.cpp:56,69,364,414; all-versus-all runs also :503,509) -- for bin/comparator */
int spsp_compare_files_chatty(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query,
                              int precision, double min_threshold, const char* out_prefix, int all_versus_all);

/* The comparator over several GPUs of one node (the reference's compare_sketches, Comparator.cpp:39-74, is
 * one thread over one merge).  One context per entry of `devices` (the same device may be named more than once: contexts
 * then share it), one host thread each.  The split is by KEY: every context decodes a block of the sketch files, deals
 * its keys into one exchange slot per context (spsp_partition_keys_device: equal keys hash to the same slot), fetches
 * the slots of its own hash class from all the others (peer copies over xGMI), compares ALL sketches' keys of that class
 * (spsp_compare_slots_device: 1/n_dev of the dictionary and of the row sums, the same share for every context) and
 * hands the non-zero cells of its partial matrix to the host (spsp_matrix_cells_device), where they add up to the pair
 * matrix the two CSVs are printed from.  Same files out as spsp_compare_files, byte for byte.
 * chatter: 0 silent, 1 / 2 the reference's stdout lines of an all-versus-all / a query run (spsp_compare_files_chatty);
 * times (may be NULL): wall seconds per stage. */
int spsp_compare_files_multi(const int* devices, uint32_t n_dev, const char* const* paths, uint32_t n, uint32_t n_query, int precision,
                             double min_threshold, const char* out_prefix, int chatter, struct spsp_stage_times* times);

/* Sketches of different sampling rates (not in the reference, which keeps the last header's rate in a member nobody reads,
 * Comparator.cpp:23-37, and so compares a -s 100 sketch with its -s 1000 twin at a Jaccard index near 0.1).  A k-mer is
 * selected iff XXH64 (seed 1312) of its canonical minimizer is <= spsp_threshold_host(k, m, s), and nothing else in the scan
 * depends on the threshold: the keys of the sketch at a coarser rate s' >= s are exactly the keys of the sketch at s whose
 * minimizer passes the threshold of s'.  Opt-in: without a rate everything below behaves as the reference does.
 *
 * spsp_keys_downsample_device keeps the keys whose minimizer passes `threshold`: sketches stay back to back, each one's
 * surviving keys in their old order (sorted input stays sorted, SPSP_KEYS_UNORDERED input stays distinct).  Input: the
 * concatenated key arrays every comparison entry point takes (they may be this context's own, e.g. what
 * spsp_sketch_decode_device or spsp_sketch_keys_device returned, or the result of the previous downsample call).  Output:
 * arrays OWNED BY THE CONTEXT, valid until the next downsample call but one on it (two sets are used in turn), ready for
 * spsp_compare_device / spsp_compare_cells_device / spsp_partition_keys_device; sk_off_out gets n + 1 offsets starting at 0.
 * A fixed chain of launches whatever n is and one host synchronisation (the one that reads the offsets back). */
int spsp_keys_downsample_device(spsp_ctx* ctx, uint32_t k, uint64_t threshold, const void* d_minimizer, const void* d_kmer_lo,
                                const void* d_kmer_hi /* NULL if k <= 32 */, const uint64_t* h_sk_off, uint32_t n,
                                void** d_out_minimizer, void** d_out_kmer_lo, void** d_out_kmer_hi, uint64_t* sk_off_out /* n + 1 */);
/* The four fields of a sketch's header line "<2k-m> <m> <count> <rate>\n" (rate by strtod: -s is a float, printed with %f).
 * A header without a rate field is SPSP_ERR_FORMAT. */
int spsp_sketch_header_host(const uint8_t* payload, uint64_t len, uint32_t* k, uint32_t* m, uint64_t* n_kmers, double* rate);
/* A sketch payload brought down to the coarser `rate`: the buckets whose minimizer passes spsp_threshold_host(k, m, rate),
 * copied as they are and in their order, behind a new header line that names `rate`.  The header's third field -- read by
 * nobody (Comparator.cpp:31); the sketcher writes its selected k-mer occurrences there -- is the number of DISTINCT keys the
 * kept buckets decode to (what spsp_sketch_parse_host returns for the result).  Rates are compared as the thresholds they
 * stand for: a `rate` finer than the sketch's own is SPSP_ERR_ARG ("cannot upsample"), one equal to it returns the payload
 * unchanged.  *out is released with spsp_free(). */
int spsp_sketch_downsample_host(const uint8_t* payload, uint64_t len, double rate, uint8_t** out, uint64_t* out_len);
/* The comparator drivers with a common sampling rate.  rate = SPSP_RATE_AS_IS: spsp_compare_files(_chatty) / _multi, which are
 * calls of these.  Otherwise every header's rate is read, and the decoded keys are brought down to the common rate ON THE
 * DEVICE, between the decoder and the comparison (between each context's decode and its key partition in the multi form: a
 * filtered key never crosses the fabric); card[i] counts the surviving keys, so both CSVs are those of sketches made at the
 * common rate directly.  "Coarser" and "already there" are decided on spsp_threshold_host(k, m, rate) of the rates, not on
 * the floats as printed; when every sketch is already at the common rate the pass is skipped.  A sketch coarser than the
 * common rate is SPSP_ERR_ARG naming the file and both rates, before any kernel runs; files of differing k or m are
 * SPSP_ERR_FORMAT naming the file; k == m collections (the phantom key of spsp_sketch_chain_host has no meaning under a
 * filter) are SPSP_ERR_ARG.  chatter: 0 silent, 1 / 2 the reference's stdout lines of an all-versus-all / a query run, and
 * behind them one line that names the common rate and how many sketches were brought down to it. */
#define SPSP_RATE_AS_IS 0.0       /* the headers' rates are ignored, as the reference does */
#define SPSP_RATE_COARSEST (-1.0) /* the largest rate any of the n headers names */
int spsp_compare_files_rate(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, double min_threshold,
                            const char* out_prefix, int chatter, double rate);
int spsp_compare_files_multi_rate(const int* devices, uint32_t n_dev, const char* const* paths, uint32_t n, uint32_t n_query, int precision,
                                  double min_threshold, const char* out_prefix, int chatter, struct spsp_stage_times* times, double rate);

/* A pair matrix in sparse form: the non-zero cells (i, j > i) of rows row_first <= i < row_limit of the dense n x n
 * matrix d_inter as packed 64-bit words  i << 48 | j << 32 | count  (n <= 65535, the reference's bound: Comparator.h:26),
 * in no particular order, in d_cells (room for `cap` words).  *n_cells = how many there are; SPSP_ERR_OVERFLOW when
 * that is more than cap (nothing is lost: call again with that much room).  A partial matrix of the key-partitioned
 * split is mostly zeros -- this is what crosses the fabric instead of n x n cells.  Waits for the context's stream. */
int spsp_matrix_cells_device(spsp_ctx* ctx, const void* d_inter, uint32_t n, uint32_t row_first, uint32_t row_limit, void* d_cells,
                             uint64_t cap, uint64_t* n_cells);
/* spsp_compare_device (every row i < n_query, all-vs-all: n_query = n) and spsp_compare_slots_device with the result
 * returned in that sparse form.  Where the comparison's form allows it -- the partition form, all rows, one workgroup
 * per row: every large problem -- the cells leave the row sums directly and the dense matrix is never written (d_scratch,
 * n x n uint32, stays as it was); otherwise d_scratch receives the dense matrix and is sparsified.  SPSP_ERR_OVERFLOW
 * with *n_cells = the room needed when there are more than cap.  Synchronous. */
int spsp_compare_cells_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi,
                              const uint64_t* h_sk_off, uint32_t n, uint32_t n_query, void* d_scratch, void* d_cells, uint64_t cap,
                              uint64_t* n_cells);
int spsp_compare_slots_cells_device(spsp_ctx* ctx, uint32_t k, const void* d_slots, uint32_t parts, uint32_t n, uint32_t slot_cap,
                                    void* d_scratch, void* d_cells, uint64_t cap, uint64_t* n_cells);
/* d_inter[i][j] += count for every packed cell (the collecting side of the above) */
int spsp_matrix_add_cells_device(spsp_ctx* ctx, void* d_inter, uint32_t n, const void* d_cells, uint64_t n_cells);

/* ------------------------------------------------------------- gather ---- */
/* Which references make up a query sketch (not in the reference, whose comparator -q stops at one row of containment numbers:
 * ten strains that share their k-mers with the one strain in the sample all score 0.9 there).  Greedy, on sets of the
 * comparator's keys, integers only.  Q = the keys of one query, R_0 .. R_{N-1} those of the references in list order, A_0 = Q;
 * round r = 1, 2, ...: u_j = |R_j n A_{r-1}|; j* = the SMALLEST j among those with the largest u_j; stop if u_j* < min_keys,
 * or if max_rounds > 0 and r > max_rounds; else emit the row below and A_r = A_{r-1} \ R_j*.  A reference is named at most
 * once, unique <= intersect, `unique` never grows down a query's rows, and |Q| - sum(unique) = the last row's `remaining`.
 * Several queries are gathered independently against the same references. */
typedef struct spsp_gather_row {
    uint32_t query;      /* index of the query sketch (< n_query) */
    uint32_t rank;       /* r: 1 for the query's first row */
    uint32_t match;      /* j* as the sketch's index in the call's list (>= n_query) */
    uint32_t reserved;   /* 0 */
    uint64_t intersect;  /* |R_j* n Q| */
    uint64_t unique;     /* u_j*: keys nobody named before it explains */
    uint64_t remaining;  /* |A_{r-1}| - u_j*: keys of the query still unexplained behind this row */
} spsp_gather_row;

/* Input: the concatenated key arrays every comparison entry point takes, SORTED per sketch as the decoder leaves them
 * ((minimizer, kmer_hi, kmer_lo) ascending: the match is a binary search), the n_query queries first, the references behind
 * them -- the layout of query mode.  The arrays are only read (the decoder's and the downsampler's stay as they are); the
 * work buffers belong to the context and are reused call after call.  Rows come back ordered by (query, rank); a query that
 * names nobody has none.  More rows than `cap`: SPSP_ERR_OVERFLOW with *n_rows = the room needed and `rows` untouched.
 * SPSP_ERR_ARG for n_query == 0, n_query >= n, min_keys == 0, n > 65535, keys that are not strictly increasing inside a
 * sketch, and on a context switched to unordered keys (spsp_compare_keys_unordered).  Launches: one match pass over the
 * reference keys per query (one launch), two scans, one fill, then two small launches per round queued in batches of 32,
 * 64, 128, ... rounds for all queries at once; the host waits once for the match count and once per batch, never per round. */
int spsp_gather_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi /* NULL if k <= 32 */,
                       const uint64_t* h_sk_off, uint32_t n, uint32_t n_query, uint64_t min_keys, uint32_t max_rounds,
                       spsp_gather_row* rows, uint64_t cap, uint64_t* n_rows);
/* The rows as text: the line "query,rank,match,intersect,unique,f_unique_query,f_match,remaining", then one line per row --
 * names[query] and names[match] as they stand, the integers in decimal, f_unique_query = unique / card[query] and f_match =
 * intersect / card[match] as IEEE double divisions printed as the matrices print a score (%.<precision>g).  card[i] = the key
 * count of sketch i as the gather saw it.  No rows: the header line alone.  A row that names a sketch outside the lists, or a
 * query as a match, is SPSP_ERR_ARG.  *text is released with spsp_free(). */
int spsp_gather_csv_host(const spsp_gather_row* rows, uint64_t n_rows, const char* const* names, uint32_t n, uint32_t n_query,
                         const uint64_t* card, int precision, char** text, uint64_t* len);
/* The whole-file driver: the files are read, inflated and decoded as spsp_compare_files_rate does it (the same code), with the
 * same `rate` argument -- SPSP_RATE_AS_IS, a rate, or SPSP_RATE_COARSEST; the downsampling pass then runs between the decoder
 * and the match, and card counts the surviving keys -- and the same refusals (a file coarser than the common rate, differing k
 * or m); k == m collections are SPSP_ERR_ARG with and without a rate (their phantom key has no meaning here).  Writes ONE file,
 * <out_prefix>_gather.csv.gz (gzip level 1, as the matrices), and no matrices.  chatter != 0: the reference's "kmers evaluated"
 * line, then one line per query -- how many references were named, how many keys remain -- and the common-rate line when a
 * rate was asked for.  rows (may be NULL) receives a copy of the rows, released with spsp_free(); n_rows may be NULL. */
int spsp_gather_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, uint64_t min_keys,
                      uint32_t max_rounds, const char* out_prefix, int chatter, double rate,
                      spsp_gather_row** rows /* may be NULL; spsp_free */, uint64_t* n_rows);

/* ------------------------------------------------------------ cluster ---- */
/* Which sketches of a collection are the same thing, and which one to keep of each group (not in the reference, whose end
 * product is the two n x n matrices).  Single linkage, on the comparator's keys, integers only.  Sketches are 0 .. n-1 in list
 * order, c_i = the key count of sketch i, x_ij = the keys i and j share; the threshold is the fraction num / den with
 * 1 <= num <= den <= 1 000 000.  i < j are LINKED iff x_ij >= 1 and
 *     SPSP_CLUSTER_JACCARD      x_ij * den >= num * (c_i + c_j - x_ij)
 *     SPSP_CLUSTER_CONTAINMENT  x_ij * den >= num * min(c_i, c_j)            (the larger of the two containment indices)
 * (equality passes; no floating point takes part).  A cluster is a connected component of that graph.  Clusters are numbered
 * 0, 1, 2, ... in the order of their first-listed member (sketch 0 is in cluster 0); a sketch without an edge is a cluster of
 * one; two empty sketches are never linked (no cell names them).  The representative of a cluster is its member with the most
 * keys, the first listed among equals. */
#define SPSP_CLUSTER_JACCARD 0
#define SPSP_CLUSTER_CONTAINMENT 1
typedef struct spsp_cluster_row {   /* one per sketch, in list order; 24 bytes */
    uint32_t cluster;         /* number of the sketch's cluster */
    uint32_t representative;  /* index of that cluster's representative */
    uint32_t size;            /* members of the cluster */
    uint32_t reserved;        /* 0 */
    uint64_t shared;          /* x_{i,representative}; c_i for the representative itself.  May be 0: single linkage chains, and
                                 a member need not touch its representative */
} spsp_cluster_row;

/* d_cells: n_cells packed words i << 48 | j << 32 | count on the device, what spsp_compare_cells_device or
 * spsp_matrix_cells_device leaves there (every pair at most once, any order, i < j < n <= 65535, count <= min(c_i, c_j)); they
 * are only read.  h_card: the n key counts (host), each below 2^47.  rows receives n rows; *n_clusters the number of clusters,
 * *n_edges the number of pairs that passed the threshold.  The work buffers belong to the context and are reused call after
 * call.  A fixed chain of launches whatever n and n_cells are -- init, link (a lock-free union per edge), flatten, a scan over
 * the "is a root" flags, a second pass over the cells for `shared`, rows -- and ONE host wait at the end.  SPSP_ERR_ARG, before
 * any kernel runs, for n == 0, n > 65535, a metric other than the two, num == 0, num > den, den > 1 000 000 and a key count of
 * 2^47 or more; SPSP_ERR_ARG also for a cell with i >= j or j >= n (found by the link kernel, which never indexes with such a
 * pair).  n_cells == 0 is valid: n clusters of one. */
int spsp_cluster_cells_device(spsp_ctx* ctx, const void* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n,
                              int metric, uint32_t num, uint32_t den,
                              spsp_cluster_row* rows /* n */, uint64_t* n_clusters, uint64_t* n_edges);
/* The rows as text: the line "sketch,cluster,representative,size,keys,shared,score", then one line per sketch in list order --
 * names[i], cluster, names[representative], size, card[i], shared in decimal, and score = the metric's value for (i,
 * representative) as an IEEE double division (shared / (card[i] + card[representative] - shared), or shared / min of the two
 * counts; 0 when shared is 0) printed as the matrices print a score (%.<precision>g); a representative's own row prints 1.
 * The score is only printed: it never decided anything.  A row that names a representative >= n, or one outside its own
 * cluster, is SPSP_ERR_ARG.  *text is released with spsp_free(). */
int spsp_cluster_csv_host(const spsp_cluster_row* rows, const char* const* names, uint32_t n, const uint64_t* card,
                          int metric, int precision, char** text, uint64_t* len);
/* The whole-file driver: the files are read, inflated and decoded as spsp_compare_files_rate does it (the same code), with the
 * same `rate` argument (SPSP_RATE_AS_IS, a rate, or SPSP_RATE_COARSEST) and the same refusals; then the all-vs-all as cells, for
 * every n, and the cluster pass.  The cells never leave the device: the n rows and the two counts come back.  Writes ONE file,
 * <out_prefix>_clusters.csv.gz (gzip level 1, as the matrices), and no matrices.  k == m collections are SPSP_ERR_ARG.
 * chatter != 0: the reference's "kmers evaluated" line, one line with sketches, edges, clusters and the largest cluster, and
 * the common-rate line when a rate was asked for.  One device: there is no multi-device form. */
int spsp_cluster_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num, uint32_t den,
                       const char* out_prefix, int chatter, double rate,
                       spsp_cluster_row** rows /* may be NULL; spsp_free */, uint64_t* n_clusters /* may be NULL */);

/* ---------------------------------------------------- representatives ---- */
/* Greedy dereplication: the other answer to "which one do I keep" (not in the reference).  Single linkage chains, and a member
 * need not touch its representative; this rule promises that NO TWO REPRESENTATIVES ARE LINKED and that EVERY MEMBER IS LINKED
 * TO THE REPRESENTATIVE IT IS FILED UNDER.  On the comparator's keys, integers only.  Sketches are 0 .. n-1 in list order, c_i =
 * the key count of sketch i, x_ij = the keys i and j share, the threshold is num / den with 1 <= num <= den <= 1 000 000, and
 * w_i is a caller-given weight, 0 <= w_i < 2^47 (genome quality, say); without weights w_i = c_i.
 *   1. LINK: the cluster pass's rule, to the letter (SPSP_CLUSTER_JACCARD / SPSP_CLUSTER_CONTAINMENT above; equality passes; two
 *      empty sketches are never linked).
 *   2. ORDER: a comes before b iff w_a > w_b, or w_a == w_b and a < b.
 *   3. REPRESENTATIVES: going through the sketches in that order, a sketch is a representative iff it is linked to no
 *      representative before it.  (The lexicographically first maximal independent set of the link graph: unique.)
 *   4. ASSIGNMENT: a sketch that is not a representative goes to the best of the representatives it is linked to: p is better
 *      than q iff x_p * u_q > x_q * u_p (128-bit products), u = c_i + c_p - x or min(c_i, c_p), the metric's denominator for the
 *      pair; where the two fractions are equal, the representative that comes first in the order of 2.  At least one of the
 *      representatives it is linked to comes before it; the best one need not.
 *   5. ROWS: one spsp_cluster_row per sketch.  Clusters are numbered 0, 1, 2, ... in the order of their first-listed member;
 *      size = the members filed under the representative, itself included; shared = x_{i,representative}, here always >= 1, and
 *      c_i for the representative itself.
 *
 * d_cells, h_card: as spsp_cluster_cells_device takes them; the cells are only read.  h_weight: n weights (host), or NULL for the
 * key counts.  rows receives n rows, *n_clusters the number of representatives, *n_edges the number of links, *n_rounds (may be
 * NULL) the rounds the selection took.  Launches: init, edges (the links as one 32-bit word each, appended per wave), rounds of
 * two small launches each (over the edges: a representative puts its later neighbours out, an undecided sketch blocks them;
 * over the sketches: undecided and not blocked becomes a representative) queued in batches of 32, 64, ..., 1024 with ONE host
 * wait per batch, then assign (a second pass over the cells: the best candidate per member by a 64-bit CAS), number, scan, rows
 * and one last wait.  The rounds needed are the depth of the order's dependency chain: about ten on random graphs, up to n on a
 * path that follows the order.  The work buffers belong to the context and are reused call after call.
 * SPSP_ERR_ARG, before any kernel runs, for what spsp_cluster_cells_device refuses and for a weight of 2^47 or more;
 * SPSP_ERR_ARG also for a cell with i >= j or j >= n (found by the edge kernel, which never indexes with such a pair): the rows
 * are then zeroed.  n_cells == 0 is valid: n clusters of one. */
int spsp_representatives_cells_device(spsp_ctx* ctx, const void* d_cells, uint64_t n_cells, const uint64_t* h_card,
                                      const uint64_t* h_weight /* NULL: the key counts */, uint32_t n, int metric, uint32_t num,
                                      uint32_t den, spsp_cluster_row* rows /* n */, uint64_t* n_clusters, uint64_t* n_edges,
                                      uint32_t* n_rounds /* may be NULL */);
/* The whole-file driver: spsp_cluster_files with this rule in place of single linkage -- the same loading, rate argument and
 * refusals (k == m collections are SPSP_ERR_ARG), the all-vs-all as cells, the pass above, and spsp_cluster_csv_host for the text:
 * the same columns.  Writes ONE file, <out_prefix>_representatives.csv.gz (gzip level 1).  h_weight: n weights, or NULL.
 * chatter != 0: the reference's "kmers evaluated" line, one line with sketches, edges, representatives, the largest cluster and
 * the rounds, and the common-rate line when a rate was asked for.  One device: there is no multi-device form. */
int spsp_representatives_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num,
                               uint32_t den, const uint64_t* h_weight /* NULL or n */, const char* out_prefix, int chatter,
                               double rate, spsp_cluster_row** rows /* may be NULL; spsp_free */,
                               uint64_t* n_clusters /* may be NULL */);

/* --------------------------------------------------------- neighbours ---- */
/* What the closest things to a sketch are: per sketch (or per query against a bank) the best few partners at or above a
 * threshold, best first (not in the reference, whose end product is the two n x n matrices).  On the comparator's keys,
 * integers only.  Sketches are 0 .. n-1 in list order, c_i = the key count of sketch i, x = the keys two sketches share.
 * ROWS AND PARTNERS.  n_query == n: every sketch is a row and all other sketches are its partners (one cell serves both of its
 * ends).  1 <= n_query < n, the queries listed first: the rows are the queries 0 .. n_query-1, their partners the references
 * n_query .. n-1; a cell between two queries (or between two references) is ignored.
 * SCORE of partner p for row r, the fraction x / u:
 *     SPSP_NEIGHBOUR_JACCARD      u = c_r + c_p - x
 *     SPSP_NEIGHBOUR_CONTAINMENT  u = min(c_r, c_p)      (the larger of the two containment indices, as clustering takes it)
 *     SPSP_NEIGHBOUR_CONTAINED    u = c_r                (the row's containment in the partner: what the containment CSV
 *                                                         prints at (r, p); not symmetric: one cell, two scores)
 * PASS.  A partner passes for a row iff x >= 1 and x * den >= num * u, with 0 <= num <= den <= 1 000 000 (num == 0: any shared
 * key passes; equality passes).
 * ORDER.  p comes before q for row r iff x_p * u_q > x_q * u_p (128-bit products); where the two are equal, the partner listed
 * first.  That is a strict total order: a row's answer is a property of the set of its passing partners.  No floating point
 * takes part: two different fractions that round to one double are still told apart. */
#define SPSP_NEIGHBOUR_JACCARD 0
#define SPSP_NEIGHBOUR_CONTAINMENT 1
#define SPSP_NEIGHBOUR_CONTAINED 2
typedef struct spsp_neighbour_row {   /* 24 bytes */
    uint32_t sketch;     /* the row: a sketch (n_query == n) or a query (< n_query) */
    uint32_t rank;       /* 1 for the row's best partner */
    uint32_t neighbour;  /* the partner's index in the call's list */
    uint32_t reserved;   /* 0 */
    uint64_t shared;     /* x: the keys the two share */
} spsp_neighbour_row;

/* d_cells: n_cells packed words i << 48 | j << 32 | count on the device, what spsp_compare_cells_device or
 * spsp_matrix_cells_device leaves there (every pair at most once, any order, i < j < n <= 65535, count <= min(c_i, c_j)); they
 * are only read.  h_card: the n key counts (host), each below 2^47.  Per row the first `top` (1 .. 64) passing partners in the
 * order above; rows come back sorted by (sketch, rank), a row without a passing partner has none.  passing (min(n, n_query)
 * words, may be NULL) receives per row how many partners passed -- more than `top` says the list was cut; *n_pairs the cells
 * with at least one passing end, each counted once.  More rows than `cap`: SPSP_ERR_OVERFLOW with *n_rows = the room needed
 * and `rows` untouched (passing and *n_pairs are already right).  The work buffers belong to the context and are reused call
 * after call.  A fixed chain of launches whatever n, n_cells and top are -- init, count, cap, two scans, fill, select -- and
 * TWO host waits: one for the two totals that size the candidate list and the rows, one for the rows.
 * SPSP_ERR_ARG, before any kernel runs, for n == 0, n > 65535, n_query == 0, n_query > n, a metric other than the three,
 * num > den, den > 1 000 000, top == 0, top > 64, a key count of 2^47 or more, and for a cell list long enough that the
 * candidates of all rows could number 2^32 or more (n_cells >= 2^31 all versus all, >= 2^32 in query mode: their places come
 * from a 32-bit scan, which must not wrap).  SPSP_ERR_ARG also for a cell with i >= j or j >= n (found by the count kernel,
 * which never indexes with such a pair); the `cap` rows and `passing` are then zeroed.  n_cells == 0 is valid: no rows. */
int spsp_neighbours_cells_device(spsp_ctx* ctx, const void* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n,
                                 uint32_t n_query, int metric, uint32_t num, uint32_t den, uint32_t top,
                                 spsp_neighbour_row* rows, uint64_t cap, uint64_t* n_rows,
                                 uint32_t* passing /* min(n, n_query) words, may be NULL */, uint64_t* n_pairs);
/* The rows as text: the line "sketch,rank,neighbour,shared,keys,neighbour_keys,score,passing", then one line per row --
 * names[sketch], rank, names[neighbour], shared, card[sketch], card[neighbour] and passing[sketch] in decimal, and score =
 * shared / u as an IEEE double division printed as the matrices print a score (%.<precision>g).  The score is only printed: it
 * never decided anything.  passing == NULL prints 0 there.  No rows: the header line alone.  A row that names a sketch outside
 * the lists (sketch >= n_query, neighbour >= n), a query as a neighbour in query mode, or neighbour == sketch, is
 * SPSP_ERR_ARG; so is a metric other than the three.  *text is released with spsp_free(). */
int spsp_neighbours_csv_host(const spsp_neighbour_row* rows, uint64_t n_rows, const uint32_t* passing, const char* const* names,
                             uint32_t n, uint32_t n_query, const uint64_t* card, int metric, int precision, char** text,
                             uint64_t* len);
/* The whole-file driver: the files are read, inflated and decoded as spsp_compare_files_rate does it (the same code), with the
 * same `rate` argument (SPSP_RATE_AS_IS, a rate, or SPSP_RATE_COARSEST) and the same refusals; then the rows of the first
 * n_query sketches (n_query == n: all versus all) as cells, and the neighbours pass.  The cells never leave the device.  Writes
 * ONE file, <out_prefix>_neighbours.csv.gz (gzip level 1, as the matrices), and no matrices.  k == m collections are
 * SPSP_ERR_ARG.  chatter != 0: the reference's "kmers evaluated" line, one line with sketches, passing pairs and rows written,
 * and the common-rate line when a rate was asked for.  One device: there is no multi-device form. */
int spsp_neighbours_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, int metric,
                          uint32_t num, uint32_t den, uint32_t top, const char* out_prefix, int chatter, double rate,
                          spsp_neighbour_row** rows /* may be NULL; spsp_free */, uint64_t* n_rows /* may be NULL */);

/* --------------------------------------------------------- prevalence ---- */
/* How many of the sketches hold each key (not in the reference, whose end product is the two n x n matrices: they say nothing
 * about whether one key is in 3 or in 9 000 sketches).  On the comparator's keys, integers only.  Sketches are 0 .. n-1 in list
 * order, K_i the keys of sketch i, c_i = |K_i|.  n_query == 0: all versus all -- every sketch is a row and a reference, R = n.
 * n_query > 0, the layout of query mode: the first n_query sketches are rows only, the R = n - n_query sketches behind them the
 * references.
 * HOLDER COUNT.  h(x) = the number of references j with x in K_j (all versus all: >= 1 for a row's own keys; query mode: may be 0).
 * CLASSES, exclusive, in this order, for the threshold num / den with 1 <= num <= den <= 1 000 000:
 *     absent  h == 0                                   (query mode only)
 *     core    h >= 1 and h * den >= num * R            (equality passes; 64-bit products; no floating point takes part)
 *     unique  not core and h == 1
 *     shell   everything else
 * PER ROW SKETCH i (every sketch, or every query): how many keys of K_i fall in each class -- they sum to c_i -- and
 * holders = the sum of h(x) over K_i.  All versus all, holders - c_i is row i's sum of the comparison's pair matrix; in query
 * mode holders is that row sum over the references.
 * SPECTRUM.  S[t], t = 1 .. R = the distinct keys of the references' union with h == t (queries take no part): sum S[t] = the
 * size of the union, sum t * S[t] = the references' key counts added up. */
typedef struct spsp_prevalence_row {   /* 40 bytes */
    uint64_t core, shell, unique, absent;   /* keys of the row sketch per class */
    uint64_t holders;                       /* sum of h over the row sketch's keys */
} spsp_prevalence_row;

/* Input: the concatenated key arrays spsp_gather_device takes, sorted per sketch ((minimizer, kmer_hi, kmer_lo) strictly
 * ascending), the queries first when there are any.  The arrays are only read; the work buffers belong to the context and are
 * reused call after call.  rows receives n_query rows (n rows when n_query == 0), spectrum R + 1 words with [0] = 0.
 * d_holders (may be NULL) receives a context-owned uint32 array on the device, parallel to the key arrays: h of every key
 * occurrence (entry e of the key arrays at word e).  It stays valid until the next prevalence call on the context.
 * SPSP_ERR_ARG for n == 0, n_query >= n, n > 65535, num == 0, num > den, den > 1 000 000, keys that are not strictly
 * increasing inside a sketch, and on a context switched to unordered keys (spsp_compare_keys_unordered); rows and spectrum are
 * zeroed when the keys are refused.  Launches, the same chain whatever n and the keys are: count (a lane per reference key: its
 * slot in one table in HBM, claimed by entry number and compared by the full key, plus one on the slot's counter), read back (a
 * lane per key: holders[]), rows (a workgroup per row sketch), spectrum (over the table's slots), and ONE host wait, at the
 * end, for the rows, the spectrum and the order check.  The table's size follows from the number of reference keys alone: no
 * attempt is ever repeated. */
int spsp_prevalence_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi /* NULL if k <= 32 */,
                           const uint64_t* h_sk_off, uint32_t n, uint32_t n_query /* 0: all versus all */, uint32_t num, uint32_t den,
                           spsp_prevalence_row* rows /* n_query ? n_query : n */, uint64_t* spectrum /* R + 1 words, [0] = 0 */,
                           void** d_holders /* may be NULL */);
/* The rows as text: the line "sketch,keys,core,shell,unique,absent,f_core,mean_holders", then one line per row sketch in list
 * order -- names[i], card[i] and the four class counts in decimal, f_core = core / card[i] and mean_holders = holders / card[i]
 * as IEEE double divisions printed as the matrices print a score (%.<precision>g); both print 0 when card[i] == 0.  card[i] =
 * the key count of sketch i as the prevalence pass saw it: a row whose classes do not add up to it is SPSP_ERR_ARG.  *text is
 * released with spsp_free(). */
int spsp_prevalence_csv_host(const spsp_prevalence_row* rows, uint32_t n_rows, const char* const* names, const uint64_t* card,
                             int precision, char** text, uint64_t* len);
/* The spectrum (n_ref + 1 words, [0] ignored) as text: the line "holders,keys,cumulative", then one line per t with S[t] > 0,
 * ascending -- t, S[t] and cumulative = the sum of S[u] over u >= t (64 bit): the core's size at any threshold can be read off
 * it.  *text is released with spsp_free(). */
int spsp_spectrum_csv_host(const uint64_t* spectrum, uint32_t n_ref, char** text, uint64_t* len);
/* The whole-file driver: the files are read, inflated and decoded as spsp_compare_files_rate does it (the same code), with the
 * same `rate` argument (SPSP_RATE_AS_IS, a rate, or SPSP_RATE_COARSEST) and the same refusals (a file coarser than the common
 * rate, differing k or m); k == m collections are SPSP_ERR_ARG.  Then the prevalence pass.  Writes TWO files,
 * <out_prefix>_prevalence.csv.gz and <out_prefix>_spectrum.csv.gz (gzip level 1, as the matrices), and no matrices.
 * chatter != 0: the reference's "kmers evaluated" line, one line with the references, the size of their union and the size of
 * the core, and the common-rate line when a rate was asked for.  rows (n_query ? n_query : n) and spectrum (n - n_query + 1
 * words) receive copies, released with spsp_free(); either may be NULL.  One device: there is no multi-device form. */
int spsp_prevalence_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, uint32_t num, uint32_t den,
                          const char* out_prefix, int chatter, double rate,
                          spsp_prevalence_row** rows /* may be NULL; spsp_free */, uint64_t** spectrum /* may be NULL; spsp_free */);

/* ------------------------------------------------------- linkage tree ---- */
/* The single-linkage hierarchy of a collection, once, instead of one clustering per guessed threshold (not in the reference).
 * The single-linkage hierarchy of a graph is its maximum spanning forest: the forest's edges, best score first, are the merges,
 * and cutting them at a threshold t leaves the connected components of ALL links at t -- what spsp_cluster_cells_device reports
 * at t.  On the comparator's keys, integers only.  Sketches are 0 .. n-1 in list order, c_i = the key count of sketch i, x = the
 * keys two sketches share.
 *   1. CANDIDATES.  A cell (i < j, x) is a candidate edge iff x >= 1 and x * den >= num * u, u = c_i + c_j - x
 *      (SPSP_CLUSTER_JACCARD) or min(c_i, c_j) (SPSP_CLUSTER_CONTAINMENT): the cluster pass's link test, to the letter, at the
 *      FLOOR num / den with 0 <= num <= den <= 1 000 000, den >= 1 (num == 0: every cell that shares a key).
 *   2. ORDER.  Edge a comes before edge b iff x_a * u_b > x_b * u_a (128-bit products); where the two fractions are equal, iff
 *      (i_a, j_a) < (i_b, j_b).  A strict total order: the forest is unique, a property of the SET of cells.
 *   3. FOREST.  Going through the candidates in that order, an edge is kept iff its two ends are not yet connected by kept
 *      edges (Kruskal).  The kept edges number n - (the clusters spsp_cluster_cells_device reports at the floor).
 *   4. ROWS.  One spsp_tree_row per kept edge, in that order: the best merge first. */
typedef struct spsp_tree_row {   /* 24 bytes */
    uint32_t a, b;       /* the cell's two sketches, a < b */
    uint32_t size;       /* sketches in the merged cluster after this merge */
    uint32_t reserved;   /* 0 */
    uint64_t shared;     /* x: the keys the two share */
} spsp_tree_row;

/* d_cells, h_card: as spsp_cluster_cells_device takes them (key counts below 2^47); the cells are only read.  rows has room for
 * n - 1 rows (may be NULL when n == 1); *n_rows receives how many there are, *n_edges the candidate edges, *n_rounds (may be
 * NULL) the rounds that merged anything.  Boruvka's algorithm in the order of 2: init, edges (the candidates appended to a
 * list, one atomic per workgroup and tile), then floor(log2 n) rounds of three small launches -- pick (every edge still between two
 * components is offered to both components' best-edge words by a 64-bit CAS, and moves on to the next round's list), hook (a
 * component's best edge is written down once and the two components are united), flatten (every sketch's root) -- all queued
 * at once, and ONE host wait at the end; a round with nothing left returns at its first load.  The forest's at most n - 1
 * edges are put into the order of 2 on the host.  The work buffers belong to the context and are reused call after call.
 * SPSP_ERR_ARG, before any kernel runs, for n == 0, n > 65535, a metric other than the two, num > den, den == 0,
 * den > 1 000 000 and a key count of 2^47 or more; SPSP_ERR_ARG also for a cell with i >= j or j >= n (found by the edge kernel,
 * which never indexes with such a pair): the n - 1 rows are then zeroed.  n_cells == 0 is valid: no rows. */
int spsp_tree_cells_device(spsp_ctx* ctx, const void* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, int metric,
                           uint32_t num, uint32_t den, spsp_tree_row* rows /* n - 1 */, uint64_t* n_rows, uint64_t* n_edges,
                           uint32_t* n_rounds /* may be NULL */);
/* The clustering at a threshold, from the rows alone.  The rows of a tree built at the floor floor_num / floor_den that pass the
 * candidate test at num / den (num == 0: all of them) are taken, and their connected components numbered 0, 1, 2, ... in the
 * order of their first-listed member: cluster[i] (n words) and *n_clusters are the `cluster` column and the count of
 * spsp_cluster_cells_device at num / den on the cells the tree was built from (the cut property of a maximum spanning forest).
 * SPSP_ERR_ARG for a cut below the floor (num * floor_den < floor_num * den), either fraction outside 0 <= num <= den <=
 * 1 000 000, den >= 1, and a row that does not name a < b < n. */
int spsp_tree_cut_host(const spsp_tree_row* rows, uint64_t n_rows, uint32_t n, const uint64_t* card, int metric,
                       uint32_t floor_num, uint32_t floor_den, uint32_t num, uint32_t den, uint32_t* cluster /* n */,
                       uint64_t* n_clusters);
/* The rows as text: the line "step,a,b,shared,keys_a,keys_b,score,size,clusters", then one line per row -- step counts from 1,
 * names[a], names[b], shared, card[a], card[b] in decimal, score = shared / u as an IEEE double division printed as the matrices
 * print a score (%.<precision>g; only printed: the integer order has decided), size, and clusters = n - step: what is left after
 * the merge.  A row that does not name a < b < n, or more than n - 1 rows, is SPSP_ERR_ARG.  *text is released with spsp_free(). */
int spsp_tree_csv_host(const spsp_tree_row* rows, uint64_t n_rows, const char* const* names, uint32_t n, const uint64_t* card,
                       int metric, int precision, char** text, uint64_t* len);
/* The rows as ONE Newick tree.  A leaf is names[i] inside single quotes, an inner ' doubled, at height 0; row r's node joins the
 * clusters its two sketches are in at height h = 1.0 - (double)shared / (double)u (IEEE doubles: printed, they decide nothing);
 * a branch length is h_parent - h_child, formed in double and printed with %.<precision>g (never negative: the rows come best
 * first and correctly rounded division is monotone).  Of a node's two children the one whose subtree holds the smaller sketch
 * index comes first.  Components that never merge are joined at height 1.0 one after another in first-member order -- ((A,B),C)
 * for three of them.  n == 1: 'name';  The text ends with ";\n".  No recursion: a path of 65 535 sketches is a legal input.  A row
 * that does not name a < b < n, or one whose two sketches are joined already, is SPSP_ERR_ARG.  *text is released with
 * spsp_free(). */
int spsp_tree_newick_host(const spsp_tree_row* rows, uint64_t n_rows, const char* const* names, uint32_t n, const uint64_t* card,
                          int metric, int precision, char** text, uint64_t* len);
/* The whole-file driver: spsp_cluster_files' loading, rate argument and refusals (k == m collections are SPSP_ERR_ARG), the
 * all-vs-all as cells, the pass above.  Writes TWO files, <out_prefix>_tree.csv.gz (spsp_tree_csv_host, gzip level 1) and
 * <out_prefix>_tree.nwk (spsp_tree_newick_host, plain text), and no matrices.  chatter != 0: the reference's "kmers evaluated"
 * line, one line with sketches, candidate edges, forest rows, the components left and the rounds, and the common-rate line when
 * a rate was asked for.  rows (may be NULL) receives a copy of the rows, released with spsp_free(); n_rows may be NULL.  One
 * device: there is no multi-device form. */
int spsp_tree_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num, uint32_t den,
                    const char* out_prefix, int chatter, double rate, spsp_tree_row** rows /* may be NULL; spsp_free */,
                    uint64_t* n_rows /* may be NULL */);

/* ---------------------------------------------------------- selection ---- */
/* The keys of a collection whose holder count lies in a band, as sketches again (not in the reference): what the prevalence pass
 * counts -- core, shell, unique, absent -- and the union and the intersection beside them, written so that every comparison above
 * can read them.  Notation as for the prevalence pass: sketches 0 .. n-1, n_query == 0: every sketch is a row and a reference
 * (R = n); n_query > 0: the first n_query sketches are rows only, the R = n - n_query behind them the references; h(x) = the
 * references that hold key x.
 * BAND.  A pair h_min, h_max of unsigned 32-bit numbers: a key passes iff h_min <= h(x) <= h_max.  h_min > h_max is a valid, empty
 * band.  Nothing else decides.
 * EACH (merged == 0).  Every row sketch keeps its passing keys in their old order: n_rows = (n_query ? n_query : n) sketches back
 * to back and n_rows + 1 offsets.
 * MERGED (merged != 0).  The distinct keys of the references' union that pass, strictly increasing by (minimizer, kmer_hi,
 * kmer_lo): ONE sketch, two offsets.  Queries take no part (n_query must be 0) and h == 0 cannot occur.
 *
 * Input: the concatenated sorted key arrays every comparison takes (the decoder's, the downsampler's, or an earlier selection's);
 * they are only read.  Output: arrays OWNED BY THE CONTEXT, valid until the next select call but one on it (two sets are used in
 * turn: a selection may read the one before it), distinct from the decoder's, the downsampler's and the prevalence pass's
 * buffers, ready for spsp_compare_device, spsp_gather_device, spsp_prevalence_device and a further select.  The call uses the
 * prevalence pass's table and holders[] (a d_holders pointer obtained earlier is overwritten).
 * SPSP_ERR_ARG for n == 0, n > 65535, n_query >= n, merged with n_query > 0, a context switched to unordered keys, and keys that
 * are not strictly increasing inside a sketch (sk_off_out is then zeroed); SPSP_ERR_OVERFLOW beyond 0xfffffff0 keys.  Launches,
 * the same chain whatever the keys are: the prevalence pass's table fill (memset, count, read back), a flag kernel over holders[]
 * (one ballot word per 64 keys, one count per tile of 2048), the downsampling pass's compaction (scan, move, offsets) and ONE host
 * wait for the offsets; merged: the read-back also marks the one occurrence that claimed each key's slot, only those are flagged,
 * and the compacted keys are sorted as one segment behind that wait (the count sizes the sort), with the sort's own wait. */
int spsp_keys_select_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi /* NULL if k <= 32 */,
                            const uint64_t* h_sk_off, uint32_t n, uint32_t n_query, uint32_t h_min, uint32_t h_max, int merged,
                            void** d_out_minimizer, void** d_out_kmer_lo, void** d_out_kmer_hi,
                            uint64_t* sk_off_out /* each: n_rows + 1; merged: 2 */);
/* A band from a word, for R >= 1 references (bin/comparator -S / -E and the Python interface read the same text).  Each named
 * class is the class of that name the prevalence pass counts at threshold <t>, with core_min = ceil(num * R / den):
 *     union, present   [1, R]
 *     absent           [0, 0]                                   (meaningful with queries)
 *     all              [R, R]                                   (the intersection)
 *     core=<t>         [core_min, R]
 *     unique=<t>       [1, 1] if core_min > 1, else empty
 *     shell=<t>        [2, core_min - 1], empty when core_min <= 2
 *     <a>..<b>         [a, b], plain unsigned 32-bit integers   (a > b: empty)
 * <t> is a decimal in (0, 1] with at most six digits behind the point, read as text into num / 10^digits as -c and -P read
 * theirs.  An empty band is returned as [1, 0].  Anything else is SPSP_ERR_ARG. */
int spsp_select_band_host(const char* what, uint32_t R, uint32_t* h_min, uint32_t* h_max);
/* A sketch payload from n keys, sorted and distinct ((minimizer, kmer_hi, kmer_lo) strictly increasing; k-mers canonical, as every
 * key array above holds them).  Header "<2k-m> <m> <n> <rate>\n" with the rate printed as the sketcher prints it; one bucket per
 * distinct minimizer, ascending: its m letters, a zero blob size (no maximal super-k-mers), per key ONE non-maximal super-k-mer of
 * exactly k bases as "prefix\nsuffix\n", and the closing "\n\n".  A k-mer is written in the orientation in which the minimizer's
 * value occurs literally (the canonical one when both hold it), split at its first occurrence there, so that the reader rebuilds
 * exactly that k-mer: spsp_sketch_parse_host of the payload returns the keys that went in.  About k - m + 2 bytes per key before
 * gzip; keys are NOT compacted into maximal super-k-mers.  SPSP_ERR_ARG for k == m, for keys out of order, and for a key whose
 * minimizer occurs in neither orientation of its k-mer (the message names the key's index).  *payload is released with
 * spsp_free(). */
int spsp_sketch_from_keys_host(uint32_t k, uint32_t m, double rate, const uint32_t* minimizer, const uint64_t* kmer_lo,
                               const uint64_t* kmer_hi /* NULL if k <= 32 */, uint64_t n, uint8_t** payload, uint64_t* len);
/* The whole-file driver: the files are read, inflated and decoded as spsp_prevalence_files does it, with the same `rate` argument
 * and refusals (k == m collections are SPSP_ERR_ARG), the band `what` is read by spsp_select_band_host for R = n - n_query, the
 * selection runs, and the selected keys are written by spsp_sketch_from_keys_host at gzip level 9, as the sketcher writes.
 * each == 0 (merged; n_query must be 0): ONE file, <out_prefix>_select.gz.  each != 0: one file per row sketch i,
 * <out_prefix>_<i>_<basename of paths[i]>, and <out_prefix>_select.txt, which lists them in order -- a file of files for -f / -q.
 * The rate written into the headers: the common rate when one was asked for; else the headers' own rate if they all stand for one
 * selection threshold; else SPSP_ERR_ARG ("sketches of different rates: give a rate").  chatter != 0: the reference's "kmers
 * evaluated" line, one line with R, the band, keys in and keys written, and the common-rate line when a rate was asked for.
 * *keys_in (the rows' keys; merged: the references') and *keys_out may be NULL.  One device: there is no multi-device form. */
int spsp_select_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, const char* what, int each,
                      const char* out_prefix, int chatter, double rate, uint64_t* keys_in /* may be NULL */, uint64_t* keys_out /* may be NULL */);

/* ------------------------------------------------------- accumulation ---- */
/* Pan and core curves (not in the reference): how the union and the intersection of a collection move as its sketches are added
 * one by one, over n_orders orders of them.  Sketches 0 .. n-1 in list order with key sets K_i, 1 <= n <= 65535; there are no
 * queries.  An order is a permutation pi of 0 .. n-1, pi[j-1] the sketch added at step j = 1 .. n:
 *   pan(j)  = |K_pi[0] u ... u K_pi[j-1]|        core(j) = |K_pi[0] n ... n K_pi[j-1]|
 * Row j-1 holds, over the 1 <= n_orders <= 1024 orders, the minimum, the maximum and the 64-bit sum of both at step j, and both
 * for order 0.  Every value is a count of keys: no floating point decides anything. */
typedef struct spsp_accumulation_row {   /* 64 bytes */
    uint64_t pan_min, pan_max, pan_sum, core_min, core_max, core_sum, pan_first, core_first;
} spsp_accumulation_row;
/* The orders a seed names, for ever: order 0 is the list order; orders 1 .. n_orders-1 are Fisher-Yates shuffles of the identity
 * (for i = n-1 down to 1: j = below(i + 1); swap(a[i], a[j])) drawn one after another from ONE splitmix64 stream of state `seed`:
 * s += 0x9E3779B97F4A7C15; z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^= z >> 31.
 * below(b) draws again while z >= 2^64 - (2^64 mod b) and returns z mod b.  orders: n_orders x n words, order p at p * n. */
int spsp_accumulation_orders_host(uint32_t n, uint32_t n_orders, uint64_t seed, uint32_t* orders /* n_orders * n */);
/* What the device call runs with for n sketches (any pointer may be NULL): the orders one pass over the keys serves (group: a
 * power of two, 8 at the most), the ranks one window of the first-rank histogram covers (n while group orders and all n bins fit
 * the LDS, which they do up to n = 25 941; beyond that one order per pass and ceil(n / window) windows), the ranks one pass of a
 * long list's mex marks, and the list length above which the whole wave walks a list instead of one lane. */
int spsp_accumulation_plan_host(uint32_t n, uint32_t* group, uint32_t* window, uint32_t* bitmap_bits, uint32_t* cut);
/* The curves of the sketches 0 .. n-1 over concatenated sorted key arrays on the device (as spsp_prevalence_device takes them; only
 * read) for the given orders (host, n_orders x n; any permutations: spsp_accumulation_orders_host's or a caller's own).  rows: n
 * rows, row j-1 is step j.  pan, core (either may be NULL): n_orders x n words, the curve of order p at p * n.  Built once per
 * call: the prevalence pass's table fill (its table and holders[] are overwritten) and the key-major form of the collection -- per
 * distinct key the list of its holders; then one streaming pass over that form per group of orders, whose rank tables sit in LDS.
 * One host wait, at the end.  SPSP_ERR_ARG (rows, pan and core zeroed): n or n_orders out of range, an order that is not a
 * permutation (the message names the order and the position), k outside 1..63, decreasing offsets, a context switched to
 * unordered keys, keys out of order or twice inside a sketch; SPSP_ERR_OVERFLOW: an extent above 0xfffffff0. */
int spsp_accumulation_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi /* NULL if k <= 32 */,
                             const uint64_t* sk_off /* n + 1 */, uint32_t n, const uint32_t* orders, uint32_t n_orders,
                             spsp_accumulation_row* rows /* n: row j-1 is step j */, uint64_t* pan /* NULL or n_orders * n */,
                             uint64_t* core /* NULL or n_orders * n */);
/* The text of <prefix>_accumulation.csv.gz: "genomes,pan_min,pan_mean,pan_max,core_min,core_mean,core_max,new_mean,pan_listed,
 * core_listed" and one line per j = 1 .. n.  pan_mean = pan_sum / n_orders, core_mean likewise, new_mean = (pan_sum(j) -
 * pan_sum(j-1)) / n_orders with pan_sum(0) = 0: the three are printed as %.<precision>g and decide nothing; the rest are integers.
 * Rows that cannot be curves are SPSP_ERR_ARG: a minimum above its maximum, a sum outside [n_orders * min, n_orders * max], pan_min
 * falling or core_max rising with j, pan_first or core_first outside [min, max].  *text is released with spsp_free(). */
int spsp_accumulation_csv_host(const spsp_accumulation_row* rows, uint32_t n, uint32_t n_orders, int precision, char** text, size_t* len);
/* The whole-file driver: the files are read, inflated and decoded as spsp_prevalence_files does it, with the same `rate` argument
 * and refusals (k == m collections are SPSP_ERR_ARG); the orders are spsp_accumulation_orders_host(n, n_orders, seed).  Writes
 * <out_prefix>_accumulation.csv.gz (gzip level 1, as the matrices) and no matrices.  rows (may be NULL) receives a copy of the n
 * rows, released with spsp_free().  One device: there is no multi-device form. */
int spsp_accumulation_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_orders, uint64_t seed, int precision,
                            const char* out_prefix, int chatter, double rate, spsp_accumulation_row** rows /* may be NULL; spsp_free */);

/* ------------------------------------------------------------- groups ---- */
/* Per-group core, exclusive and marker keys of a partitioned collection (not in the reference): what each group shares, what it
 * holds that no other group holds, and which keys identify it.  Sketches 0 .. n-1 in list order with key sets K_i, c_i = |K_i|,
 * 1 <= n <= 65535; there are no queries.  group[i] in 0 .. G-1 with 1 <= G <= n, every group with at least one member; size_c =
 * the members of group c.  h(x) = the sketches that hold key x, h_c(x) = the members of group c that hold it (sum over c of h_c = h).
 * THRESHOLDS, read as fractions; no floating point decides anything.
 *   inside   num / den,   1 <= num <= den <= 1 000 000:                   in_min_c  = ceil(num * size_c / den)          (>= 1)
 *   outside  onum / oden, 0 <= onum <= oden, 1 <= oden <= 1 000 000:      out_max_c = floor(onum * (n - size_c) / oden)
 * with 64-bit products, computed once on the host by spsp_groups_bounds_host (the device call uses that very function).
 * A key x is, for group c (counts, not a partition):
 *   present    h_c >= 1
 *   core       h_c >= in_min_c
 *   exclusive  h_c >= 1 and h_c == h                  (no holder outside c)
 *   marker     core and h - h_c <= out_max_c
 * With onum == 0 a marker is a core key nobody outside holds; with onum > 0 one key may be a marker of several groups.
 * Every number below is a property of the sets and the labels alone. */
typedef struct spsp_group_row {          /* 48 bytes, one per group */
    uint64_t members;     /* size_c */
    uint64_t entries;     /* the members' key counts added up = the sum of h_c over the present keys */
    uint64_t present, core, exclusive, marker;   /* distinct keys of each kind */
} spsp_group_row;
typedef struct spsp_group_member_row {   /* 24 bytes, one per sketch i of group c: the keys of K_i that are core, exclusive, marker of c */
    uint64_t core, exclusive, marker;
} spsp_group_member_row;
/* A labels file: one label per line in list order; "\r\n" is tolerated and the final newline is optional.  Groups are numbered by
 * first appearance: group[i] = the number of line i + 1's label, *n_groups = G.  *names (may be NULL, with names_len) receives the
 * G labels NUL-terminated back to back, released with spsp_free().  SPSP_ERR_ARG, the message naming the line: a line count
 * other than n, an empty label, a label that holds ',', '"' or a control character. */
int spsp_groups_labels_host(const char* text, uint64_t len, uint32_t n, uint32_t* group /* n */, uint32_t* n_groups, char** names /* may be NULL */,
                            uint64_t* names_len /* may be NULL */);
/* The labels and thresholds validated and the bounds above computed: size, in_min, out_max (each n_groups words, each may be NULL).
 * SPSP_ERR_ARG: n == 0 or n > 65535, n_groups == 0 or n_groups > n, a label >= n_groups, a group without a member (the message
 * names it), thresholds outside the ranges above. */
int spsp_groups_bounds_host(const uint32_t* group, uint32_t n, uint32_t n_groups, uint32_t num, uint32_t den, uint32_t onum, uint32_t oden,
                            uint32_t* size, uint32_t* in_min, uint32_t* out_max);
/* The rows of the groups and of their members over concatenated sorted key arrays on the device (as spsp_prevalence_device takes
 * them; only read).  rows: n_groups; members: n, or NULL.  want_markers != 0: the marker keys as n_groups sketches back to back --
 * group c's at [marker_off[c], marker_off[c + 1]), strictly increasing by (minimizer, kmer_hi, kmer_lo) -- in arrays OWNED BY THE
 * CONTEXT, valid until the next groups call on it, distinct from the decoder's, the downsampler's, the selection's and the
 * accumulation's buffers, ready for spsp_compare_device, spsp_gather_device, spsp_prevalence_device and spsp_keys_select_device
 * (with marker_off as their offsets).  want_markers == 0: the three pointers are set to NULL and marker_off may be NULL.
 * The call uses the prevalence pass's table and holders[] (a d_holders pointer obtained earlier is overwritten).  Launches, the
 * same chain whatever the keys are: the prevalence pass's table fill (h per entry), a second table keyed by (key, group) filled
 * and read back the same way (h_c per entry, the key's four properties for the entry's group, and one bit on the entry that
 * claimed the cell), one workgroup per sketch that counts its entries, ONE host wait, and the group rows added up on the host.
 * With markers: a flag kernel over the claimers, the downsampling pass's compaction with the sketch bounds (inside that one
 * wait), the runs moved to their groups' regions and the regions of more than one run sorted (the sort's own wait).
 * SPSP_ERR_ARG (rows, members and marker_off zeroed): what spsp_groups_bounds_host refuses, k outside 1..63, decreasing offsets, a
 * context switched to unordered keys, keys out of order or twice inside a sketch; SPSP_ERR_OVERFLOW: an extent above 0xfffffff0.
 * A refused call leaves the context usable. */
int spsp_groups_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi /* NULL if k <= 32 */,
                       const uint64_t* h_sk_off /* n + 1 */, uint32_t n, const uint32_t* h_group /* n */, uint32_t n_groups, uint32_t num, uint32_t den,
                       uint32_t onum, uint32_t oden, spsp_group_row* rows /* n_groups */, spsp_group_member_row* members /* n; may be NULL */,
                       int want_markers, void** d_out_minimizer, void** d_out_kmer_lo, void** d_out_kmer_hi,
                       uint64_t* marker_off /* n_groups + 1; may be NULL without markers */);
/* The text of <prefix>_groups.csv.gz: "group,members,keys,present,core,exclusive,marker,f_core,f_marker" and one line per group;
 * keys = entries, f_core = core / present, f_marker = marker / core.  The two quotients are IEEE doubles printed as
 * %.<precision>g, 0 on a zero denominator, and decide nothing.  SPSP_ERR_ARG for a row with core > present, marker > core or
 * exclusive > present.  *text is released with spsp_free(). */
int spsp_groups_csv_host(const spsp_group_row* rows, uint32_t n_groups, const char* const* group_names, int precision, char** text, uint64_t* len);
/* The text of <prefix>_members.csv.gz: "sketch,group,keys,core,exclusive,marker,f_core,f_marker" and one line per sketch;
 * keys = c_i (card[i]), f_core = core / c_i, f_marker = marker / the group's marker count.  SPSP_ERR_ARG for a label >= n_groups
 * and for a member row that exceeds c_i (or has marker > core) or its group's row. */
int spsp_groups_members_csv_host(const spsp_group_member_row* members, uint32_t n, const char* const* sketch_names, const uint32_t* group,
                                 const uint64_t* card, const spsp_group_row* rows, uint32_t n_groups, const char* const* group_names, int precision,
                                 char** text, uint64_t* len);
/* The whole-file driver: the files are read, inflated and decoded as spsp_prevalence_files does it, with the same `rate` argument
 * and refusals (k == m collections are SPSP_ERR_ARG); labels_path names the labels file (spsp_groups_labels_host).  Writes
 * <out_prefix>_groups.csv.gz and <out_prefix>_members.csv.gz (gzip level 1, as the matrices) and no matrices.  write_markers != 0:
 * also one sketch per group, <out_prefix>_markers_<c>.gz with <c> the group's number (spsp_sketch_from_keys_host, gzip level 9; a
 * group without a marker gets the sketch of no keys), and <out_prefix>_markers.txt, which lists them in group order -- a file of
 * files for -f / -q.  The rate written into their headers follows spsp_select_files' rule (mixed rates need a rate).  rows,
 * members (may be NULL) receive copies released with spsp_free(); *n_groups (may be NULL) = G.  One device. */
int spsp_groups_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, const char* labels_path, int precision, uint32_t num, uint32_t den,
                      uint32_t onum, uint32_t oden, int write_markers, const char* out_prefix, int chatter, double rate,
                      spsp_group_row** rows /* may be NULL; spsp_free */, spsp_group_member_row** members /* may be NULL; spsp_free */,
                      uint32_t* n_groups /* may be NULL */);

/* ------------------------------------------------------------ classify ---- */
/* The records of a sequence file assigned to the references of an index (not in the reference): which reference each contig or
 * long read belongs to, record by record.
 * INDEX: references 0 .. R-1, 1 <= R <= 65535, with sorted distinct key sets K_j: the concatenated arrays every collection pass
 * takes, refused exactly as there.  (The file driver refuses k == m collections.)
 * RECORD r has a set Q_r of distinct keys.  In the file driver Q_r is what spsp_sketch_keys_device returns for the genome made of
 * that one record with abundance = 1, scanned at spsp_threshold_host(k, m, rate): what decoding the sketch that sub_sampler writes
 * for a FASTA of that record alone would give, uint8 count rule included.  A record shorter than k, or without a selected
 * minimizer, has no keys.
 *   shared(r, j) = |Q_r n K_j|          hit_keys(r) = #{x in Q_r : some K_j holds x}
 * Reference j PASSES for r when shared >= min_keys (min_keys >= 1) and shared * den >= num * |Q_r| (64-bit products; equality
 * passes; 0 <= num <= den <= 1 000 000, 1 <= den).  passing(r) = the passing references.  The LISTED matches of r are its best
 * min(top, passing) passing references, 1 <= top <= 64, by shared descending, the lower reference number first among equals: the
 * order is total, so the answer is a function of the key sets alone.  No floating point decides anything. */
typedef struct spsp_classify_record {    /* 24 bytes, one per record */
    uint64_t length;      /* bases of the record: the caller's (the file driver fills it); the device call leaves it alone */
    uint32_t keys;        /* |Q_r| */
    uint32_t hit_keys, passing, listed;
} spsp_classify_record;
typedef struct spsp_classify_hit {       /* 8 bytes: match i of record r at hits[r * top + i], i < listed; the slots behind are zero */
    uint32_t reference, shared;
} spsp_classify_hit;
/* Builds the index of the references over concatenated sorted key arrays on the device (as spsp_prevalence_device takes them) and
 * keeps it in the context: the prevalence pass's table, filled with claimers, and the accumulation's key-major lists (per distinct
 * key the 16-bit numbers of its holders).  The caller's arrays must stay unchanged while the index is in use: the table compares
 * by full key through them.  The next prevalence, select, accumulation, groups or index call on the context replaces the index.
 * One host wait.  SPSP_ERR_ARG: n_ref outside 1 .. 65535, k outside 1..63, decreasing offsets, a context switched to unordered
 * keys, keys out of order or twice inside a reference; SPSP_ERR_OVERFLOW: an extent above 0xfffffff0. */
int spsp_classify_index_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi /* NULL if k <= 32 */,
                               const uint64_t* h_sk_off /* n_ref + 1 */, uint32_t n_ref);
/* Classifies one batch of records against the context's index.  The records' keys are distinct per record, in any order (the
 * caller vouches for "distinct"), record r's at entries [h_rec_off[r], h_rec_off[r + 1]) of arrays of the caller's on the device --
 * the key arrays of another context, a tensor, a slice; only read.  n_records is bounded by the entry extent 0xfffffff0, not by
 * 65 535.  records: n_records (length is not touched); hits: n_records * top, zero behind each record's `listed`.  Any number of
 * batches may be classified against one index; each call waits for the device once, at its end.  Launches, the same whatever the
 * records are: a probe pass (a lane per record key) that also adds up every record's work = the sum over its keys of their holders,
 * a routing pass, and the two tally-and-select forms the records were routed to by their work (spsp_classify_plan_host).
 * SPSP_ERR_ARG (records' counts zeroed, and the hits wherever `top` itself is in range): no index on the context, d_q_kmer_hi given for an index of k <= 32 or missing
 * for one of k > 32, top, min_keys, num or den out of range, decreasing offsets; SPSP_ERR_OVERFLOW: an extent above 0xfffffff0. */
int spsp_classify_device(spsp_ctx* ctx, const void* d_q_minimizer, const void* d_q_kmer_lo, const void* d_q_kmer_hi /* NULL if k <= 32 */,
                         const uint64_t* h_rec_off /* n_records + 1 */, uint32_t n_records, uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den,
                         spsp_classify_record* records /* n_records */, spsp_classify_hit* hits /* n_records * top */);
/* While the context's timing is on (spsp_timing_enable, any kind) a classify call records events between its launches; this reads
 * the milliseconds added up since the last read and clears them: ms[0] the probe pass, ms[1] the routing pass, ms[2] the wave form
 * (tally and selection are one kernel), ms[3] the workgroup form (likewise). */
int spsp_classify_stage_ms(spsp_ctx* ctx, double* ms /* 4 */);
/* What routes a record, for n_ref references and `top` matches (any pointer may be NULL).  small_work: a record whose work is at
 * most this is tallied by one wave, its holder numbers sorted and counted in LDS; a record of more work takes a workgroup with one
 * 32-bit counter per reference.  lds_refs: up to this many references those counters sit in LDS, beyond it in a row of device
 * memory per workgroup; *counters_in_lds = n_ref <= lds_refs.  list_cut: in the workgroup form a key's list of more holders than
 * this is walked by a whole wave instead of one lane.  SPSP_ERR_ARG: n_ref outside 1 .. 65535, top outside 1 .. 64. */
int spsp_classify_plan_host(uint32_t n_ref, uint32_t top, uint32_t* small_work, uint32_t* lds_refs, uint32_t* counters_in_lds, uint32_t* list_cut);
/* The text of <prefix>_classify.csv.gz: "record,name,length,keys,hit_keys,rank,match,shared,f_shared,passing" and one line per
 * listed match, rank from 1; a record without a passing reference gets one line with rank 0, an empty match, shared 0 and
 * f_shared 0.  record = the record's number from 0, match = ref_names[reference], f_shared = shared / keys as %.<precision>g (0 when
 * keys == 0; it decides nothing).  Rows that contradict themselves are SPSP_ERR_ARG, the message naming the record: listed >
 * min(top, passing), hit_keys > keys, shared > hit_keys or shared == 0 in a listed match, matches out of order (or one reference
 * twice), a reference >= n_ref.  *text is released with spsp_free(). */
int spsp_classify_csv_host(const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records, const char* const* record_names,
                           const char* const* ref_names, uint32_t n_ref, uint32_t top, int precision, char** text, uint64_t* len);
/* The text of <prefix>_classify_summary.csv.gz: "reference,records_best,bases_best,keys_best,records_listed" and one line per
 * reference -- the records whose rank-1 match it is, their lengths and shared keys added up, and the records that list it at all --
 * closed by one line named "unclassified": the records without a match, their lengths, 0 and 0.  The same refusals. */
int spsp_classify_summary_csv_host(const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records, const char* const* ref_names,
                                   uint32_t n_ref, uint32_t top, char** text, uint64_t* len);
/* The whole-file driver.  index_paths: n_ref sketch files, read, inflated and decoded as spsp_prevalence_files does it, with the
 * same `rate` argument and refusals (k == m collections are SPSP_ERR_ARG); sketches of different rates need a rate, because the
 * records are scanned at ONE threshold: spsp_threshold_host(k, m, the common rate, or the headers' own where they agree).
 * records_path: a FASTA or FASTQ file (by its first byte), gzip or plain, ingested and scanned once on a second context of the same
 * device; keys are extracted in batches of at most 65 535 records (spsp_sketch_keys_device over the records' range of the one scan)
 * and each batch is classified against the index, the two contexts ordered by spsp_wait_stream.  A record's name is the first
 * whitespace-delimited word of its header line, read on the host; a text whose headers are not as many as the records the device
 * ingest finds is SPSP_ERR_FORMAT.  Writes <out_prefix>_classify.csv.gz and <out_prefix>_classify_summary.csv.gz (gzip level 1)
 * and no matrices.  records, hits (may be NULL) receive copies released with spsp_free(); *n_records (may be NULL) their number. */
int spsp_classify_files(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys,
                        uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                        spsp_classify_record** records /* may be NULL; spsp_free */, spsp_classify_hit** hits /* may be NULL; spsp_free */,
                        uint64_t* n_records /* may be NULL */);

/* --------------------------------------------------------------- depth ---- */
/* How deep a read set covers each reference of an index (not in the reference): the one pass of the library that counts.
 * INDEX: what spsp_classify_index_device built on the context -- references 0 .. R-1 with key sets K_j, U their union, D = |U|,
 * h(x) = the references that hold key x.  The READ SET is a sequence of records r with distinct key sets Q_r, the Q_r of classify.
 *   c(x) = #{r : x in Q_r} for x in U: the records that hold x.
 * A key is FOUND at min_count >= 1 when c(x) >= min_count (2 drops the keys only a sequencing error produced).  For reference j,
 * F_j = {x in K_j : found}:  keys = |K_j|, found = |F_j|, sum = the sum of c over F_j (64 bits), max = the largest c in F_j,
 * median = the LOWER median of c over F_j: with the values ascending s_0 <= ... <= s_(found-1) it is s_floor((found-1)/2).
 * sum, max and median are 0 when found == 0.  The unique_ fields are the same five over the reference's UNIQUE keys
 * {x in K_j : h(x) == 1}: a key two strains share says nothing about which of them is in the sample.
 * Totals: record_keys = the sum of |Q_r|, hit_keys = the sum of c(x) over U, index_keys = D, index_found = #{x in U : found}.
 * Integers only: the answer is a function of the multiset of record keys, whatever the batch cuts, key order or arrival order. */
typedef struct spsp_depth_row {     /* 48 bytes, one per reference */
    uint64_t sum, unique_sum;
    uint32_t keys, found, median, max, unique_keys, unique_found, unique_median, unique_max;
} spsp_depth_row;
typedef struct spsp_depth_totals { uint64_t record_keys, hit_keys; uint32_t index_keys, index_found; } spsp_depth_totals;   /* 24 bytes */
/* Makes one 32-bit counter per distinct key of the context's index, cleared, and clears the running totals; also numbers every
 * index entry's key once (one probe per entry; one host wait, for D).  The counters belong to the index: whatever replaces or drops
 * the index (a prevalence, select, accumulation, groups or index call) ends them, and spsp_depth_add_device / _read_device are
 * SPSP_ERR_ARG until the next begin.  SPSP_ERR_ARG: no index on the context. */
int spsp_depth_begin_device(spsp_ctx* ctx);
/* Adds the keys of any number of WHOLE records: entries [first, first + n_keys) of arrays of the caller's on the device, distinct
 * per record (the caller vouches for it, as in spsp_classify_device) and otherwise in any order; no record offsets are needed.
 * One launch, a lane per record key: the probe of classify's probe pass, and on a hit one atomic add to the key's counter.  It
 * only QUEUES on the context's stream: no host wait; the arrays must stay until the stream has passed the launch.  Checked before
 * anything is queued -- SPSP_ERR_ARG: no counters on the context, d_q_kmer_hi given for an index of k <= 32 or missing for one of
 * k > 32; SPSP_ERR_OVERFLOW: n_keys > 0xfffffff0, or the record keys since begin (kept on the host in 64 bits) would pass
 * 0xffffffff -- then nothing is added, which keeps every counter from wrapping.  n_keys == 0 or an index without keys: SPSP_OK. */
int spsp_depth_add_device(spsp_ctx* ctx, const void* d_q_minimizer, const void* d_q_kmer_lo, const void* d_q_kmer_hi /* NULL if k <= 32 */,
                          uint64_t first, uint64_t n_keys);
/* The rows (n_ref, as the index has them) and the totals at min_count, with one host wait.  It does not consume the counters: it
 * may be called again, with another min_count, or between adds.  *d_entry_count (may be NULL) receives the device address of a
 * context-owned uint32 array parallel to the index's key arrays (entry e of the index at [e - h_sk_off[0]]): c of that entry's key,
 * valid until the next read, begin or index call.  Launches: a lane per index entry, then a workgroup per reference with two
 * histograms in LDS (spsp_depth_plan_host); a reference of more than 65 536 keys is reduced by segments, a workgroup each, and
 * merged.  SPSP_ERR_ARG: no counters on the context, min_count == 0. */
int spsp_depth_read_device(spsp_ctx* ctx, uint32_t min_count, spsp_depth_row* rows /* n_ref */, spsp_depth_totals* totals /* may be NULL */,
                           const void** d_entry_count /* may be NULL */);
/* *bins = the bins of one LDS histogram of the reduction: bin b < bins - 1 holds c == b, the last every c >= bins - 1; a median whose
 * rank lands in the last bin is resolved exactly by a radix select (four passes of 256 bins). */
int spsp_depth_plan_host(uint32_t* bins);
/* While the context's timing is on (spsp_timing_enable, any kind) the depth calls record events around their launches; this reads
 * the milliseconds added up since the last read and clears them (it waits for the stream where adds are outstanding): ms[0] the
 * adds, ms[1] the entry pass, ms[2] the reduction. */
int spsp_depth_stage_ms(spsp_ctx* ctx, double* ms /* 3: add, entry, reduce */);
/* The text of <prefix>_depth.csv.gz:
 * "reference,keys,found,f_found,median,mean,max,unique_keys,unique_found,f_unique_found,unique_median,unique_mean,unique_max" and
 * one line per reference; f_found = found / keys, mean = sum / found (and their unique_ forms) as %.<precision>g, 0 where the
 * denominator is 0: they decide nothing.  Rows that contradict themselves are SPSP_ERR_ARG, the message naming the reference:
 * found > keys, unique_keys > keys, unique_found > min(found, unique_keys), median > max, max > sum, found == 0 with a non-zero
 * sum, max or median, found > 0 with median == 0, sum < found or sum > found * max, the same for the unique five, unique_sum > sum.
 * *text is released with spsp_free(). */
int spsp_depth_csv_host(const spsp_depth_row* rows, const char* const* names, uint32_t n_ref, int precision, char** text, uint64_t* len);
/* The whole-file driver.  index_paths: n_ref sketch files, loaded exactly as spsp_classify_files loads them (the same `rate` rule,
 * k == m and mixed rates without a rate refused).  reads_paths: n_reads >= 1 FASTA or FASTQ files (R1 / R2, lanes), gzip or plain,
 * which go one after the other through the records path of spsp_classify_files; every batch's keys go to spsp_depth_add_device,
 * then there is one read.  Writes <out_prefix>_depth.csv.gz (gzip level 1) and no matrices; nothing on any failure.  rows (may be
 * NULL) receives a copy released with spsp_free(); totals may be NULL. */
int spsp_depth_files(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* const* reads_paths, uint32_t n_reads, uint32_t min_count,
                     int precision, const char* out_prefix, int chatter, double rate, spsp_depth_row** rows /* may be NULL; spsp_free */,
                     spsp_depth_totals* totals /* may be NULL */);

/* ------------------------------------------------------------- profile ---- */
/* Which references a read set holds, each shared key counted once, and how deep each one is (not in the reference): the greedy
 * rounds of gather on the counters of the depth pass.  Index and counts as in the depth section: references 0 .. R-1 with key sets
 * K_j, U their union, c(x) from the adds since spsp_depth_begin_device.  F = {x in U : c(x) >= min_count}, A_0 = F.
 * Round r = 1, 2, ...:  u_j = |K_j n A_(r-1)|;  j* = the SMALLEST j among the largest u_j;  stop if u_j* < min_keys, or if
 * max_rounds > 0 and r > max_rounds;  otherwise emit one row and set A_r = A_(r-1) \ K_j*.
 * The row of round r (rank = r: rows[r - 1]):  reference = j*,  keys = |K_j*|,  found = |K_j* n F| (depth's found),
 * assigned = u_j*,  sum (64 bits), median (the LOWER median, as depth defines it) and max of c(x) over x in K_j* n A_(r-1),
 * remaining = |A_(r-1)| - u_j*.  min_count >= 1 and min_keys >= 1; max_rounds = 0 means no limit; at most R rows.
 * Totals: found_keys = |F|, found_sum = the sum of c over F, assigned_keys and assigned_sum = the rows' assigned and sum added up.
 * The answer is a function of the multiset of record keys, min_count, min_keys and max_rounds: not of batch cuts, key order or the
 * order lanes meet anything in.  Integers only.  What follows, and what spsp_profile_csv_host holds rows to:
 *   assigned never increases from one row to the next;  1 <= assigned <= found <= keys;  no reference appears twice;
 *   remaining_r = remaining_(r-1) - assigned_r with remaining_0 = |F|;  assigned <= sum <= assigned * max;  1 <= median <= max;
 *   with min_keys = 1 and no round limit the last remaining is 0. */
typedef struct spsp_profile_row {   /* 40 bytes, one per round */
    uint64_t sum;
    uint32_t reference, keys, found, assigned, median, max, remaining, reserved;
} spsp_profile_row;
typedef struct spsp_profile_totals { uint64_t found_sum, assigned_sum; uint32_t found_keys, assigned_keys; } spsp_profile_totals;   /* 24 bytes */
/* The rounds on the counters of spsp_depth_begin_device / spsp_depth_add_device.  Like a read it does not consume them: any number
 * of calls, between adds, with other arguments, and a spsp_depth_read_device before or after it answers as it does without.
 * rows has room for n_ref rows, *n_rows receives their number.  *d_entry_assigned (may be NULL) receives the device address of a
 * context-owned byte array parallel to the index's key arrays: 1 where that entry's key was assigned to that entry's reference;
 * valid until the next profile, begin or index call.  Launches: the entry pass of a read and a count per reference; per round one
 * workgroup that picks (arg-max over u << 32 | ~j words) and a walk over the winner's entries that marks its live keys dead and
 * takes one off the counter of every other holder (the index's key-major lists; a list of more than 32 holders by a whole wave;
 * up to 38 912 references through counters in LDS, flushed once per workgroup);
 * then ONE run of the depth reduction with the assigned bytes in the place of the unique ones.  Rounds are queued 32, 64, 128,
 * 128, ... at a time: one host wait per batch and one for the statistics, never one per round.
 * SPSP_ERR_ARG: no counters on the context, min_count == 0, min_keys == 0.  An index without keys or an empty F: SPSP_OK, no rows. */
int spsp_profile_device(spsp_ctx* ctx, uint32_t min_count, uint32_t min_keys, uint32_t max_rounds, spsp_profile_row* rows /* n_ref */, uint64_t* n_rows,
                        spsp_profile_totals* totals /* may be NULL */, const void** d_entry_assigned /* may be NULL */);
/* While the context's timing is on the profile calls record events around their launches; this reads the milliseconds added up
 * since the last read and clears them: ms[0] the entry pass and the start, ms[1] the picks, ms[2] the walks, ms[3] the reduction. */
int spsp_profile_stage_ms(spsp_ctx* ctx, double* ms /* 4: entry + start, picks, walks, reduction */);
/* What the last spsp_profile_device call on the context did: counts[0] the rounds it queued (a stopped call's later launches
 * return at their first load), counts[1] its rows, counts[2] its host waits. */
int spsp_profile_counts(spsp_ctx* ctx, uint32_t* counts /* 3: rounds queued, rows, host waits */);
/* The text of <prefix>_profile.csv.gz:
 * "rank,reference,keys,found,f_found,assigned,f_assigned,median,mean,max,f_weighted,remaining" and one line per row, the reference
 * by its name; f_found = found / keys, f_assigned = assigned / found_keys, mean = sum / assigned, f_weighted = sum / found_sum
 * (the relative abundance) as %.<precision>g, 0 where the denominator is 0: they decide nothing.  A row that contradicts the facts
 * above (or names a reference >= n_ref, or n_rows > n_ref) is SPSP_ERR_ARG, the message naming the rank.  *text: spsp_free(). */
int spsp_profile_csv_host(const spsp_profile_row* rows, uint64_t n_rows, const spsp_profile_totals* totals, const char* const* names, uint32_t n_ref,
                          int precision, char** text, uint64_t* len);
/* The whole-file driver: the arguments of spsp_depth_files plus min_keys and max_rounds.  It loads the index and adds the reads as
 * spsp_depth_files does (the same code), then makes one read and one profile.  Writes <out_prefix>_depth.csv.gz, byte for byte what
 * spsp_depth_files writes, and <out_prefix>_profile.csv.gz; nothing on any failure.  rows, profile_rows (may be NULL) receive
 * copies released with spsp_free(); the totals may be NULL. */
int spsp_profile_files(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* const* reads_paths, uint32_t n_reads, uint32_t min_count,
                       uint32_t min_keys, uint32_t max_rounds, int precision, const char* out_prefix, int chatter, double rate,
                       spsp_depth_row** rows /* may be NULL; spsp_free */, spsp_depth_totals* totals /* may be NULL */,
                       spsp_profile_row** profile_rows /* may be NULL; spsp_free */, uint64_t* n_profile_rows /* may be NULL */,
                       spsp_profile_totals* profile_totals /* may be NULL */);

/* ------------------------------------------------------------ taxonomy ---- */
/* The records of a sequence file assigned to the lowest common ancestor of their keys (not in the reference): classify answers
 * with a reference, and a record from a region twenty strains share ties twenty ways; this answers with the node of a tree the
 * record's keys agree on.
 * TREE.  It has T nodes, with 1 <= T <= 1 048 576, numbered in preorder.  Node 0 is the root.  parent[0] = 0, parent[t] < t, and
 * every subtree is a run of consecutive numbers [t, t + size[t]).  depth[t] <= 32.  Every reference j sits at a node ref_node[j].
 * Several references may share a node.  A reference may sit at an inner node or at the root.
 * anc(a, b) means "a is b or an ancestor of b".  In this numbering that is a <= b < a + size[a].  lca(S) is the deepest node that
 * is anc of every member of S.
 * INDEX.  For every distinct key x of the index, node(x) = lca{ ref_node[j] : K_j holds x }.  This is computed once, when the
 * taxonomy is attached.
 * RECORD.  Record r has the distinct key set Q_r.  This is exactly the Q_r of classify.
 *   w(t) = the keys of Q_r found in the index whose node(x) is t.
 *   hit_keys = Sum_t w(t).
 *   path(t) = Sum_{a : anc(a, t)} w(a).
 *   clade(t) = Sum_{d : anc(t, d)} w(d).
 *   best = max{ path(t) : w(t) > 0 }.
 *   W = { t : w(t) > 0, path(t) = best }.  winners = |W|.
 *   start = lca(W).
 * A node passes when clade(t) >= min_keys and clade(t) * den >= num * |Q_r|.  The products are 64-bit and equality passes.
 * min_keys >= 1, 0 <= num <= den <= 1 000 000.
 * The call is the first passing node on the way from start to the root.  If the root does not pass either, or there is no hit, the
 * record is unclassified.  Its node is then 0xffffffff.
 * For an unclassified record node = start = 0xffffffff when there is no hit, and clade = direct = 0.  score and winners still
 * describe W.
 * Nothing depends on the order of keys in a record, of holders in a list, or of lanes. */
#define SPSP_TAXONOMY_NONE 0xffffffffu
#define SPSP_TAXONOMY_MAX_NODES 1048576u
#define SPSP_TAXONOMY_MAX_DEPTH 32u
typedef struct spsp_taxonomy_record {    /* 40 bytes, one per record */
    uint64_t length;      /* bases of the record: the caller's (the file driver fills it); the device call leaves it alone */
    uint32_t keys;        /* |Q_r| */
    uint32_t hit_keys;
    uint32_t node;        /* the call, or SPSP_TAXONOMY_NONE */
    uint32_t start;       /* lca(W), or SPSP_TAXONOMY_NONE without a hit */
    uint32_t score;       /* best */
    uint32_t clade;       /* clade(node) */
    uint32_t direct;      /* w(node) */
    uint32_t winners;     /* |W| */
} spsp_taxonomy_record;
/* A lineage file: one line per reference, in list order ("\r\n" tolerated, the final newline optional).  Each line is
 * name;name;... from below the root down to the reference's own node, as GTDB and kraken2-inspect print lineages.  Names are
 * trimmed of blanks; a name must be non-empty, without ',', '"', ';' or control characters; at most 32 names per line.  An empty
 * line puts the reference at the root.  A node is a path: the same name under two parents is two nodes.  Nodes are numbered in
 * preorder, children in order of first appearance in the file.  ref_node: n_ref words of the caller's.  *parent, *depth, *size
 * (T words each) and *names (the T names back to back, each closed by a 0 byte; node 0 is "root") are released with spsp_free();
 * any of the four may be NULL.  SPSP_ERR_FORMAT, the message naming the line: a bad name, too many names, more or fewer lines than
 * n_ref, more than 1 048 576 nodes.  SPSP_ERR_ARG: n_ref outside 1 .. 65535. */
int spsp_taxonomy_lineages_host(const char* text, uint64_t len, uint32_t n_ref, uint32_t* ref_node /* n_ref */, uint32_t** parent, uint32_t** depth,
                                uint32_t** size, char** names, uint64_t* names_len, uint32_t* n_nodes);
/* What spsp_taxonomy_index_device holds arrays of the caller's own to.  SPSP_ERR_ARG, the message naming the node or the
 * reference: T outside 1 .. 1 048 576, n_ref outside 1 .. 65535, parent[0] != 0, parent[t] >= t, a node deeper than 32,
 * ref_node[j] >= T, or a numbering that is not a preorder: parent[t] must be t - 1 or an ancestor of t - 1. */
int spsp_taxonomy_check_host(const uint32_t* parent, uint32_t n_nodes, const uint32_t* ref_node, uint32_t n_ref);
/* The cuts of the two forms for a tree of n_nodes (any pointer may be NULL).  small_hits: a record of at most this many hit keys
 * is tallied by one wave, its keys' nodes sorted in LDS; a record of more takes a workgroup with one 32-bit counter per node.
 * lds_nodes: up to this many nodes those counters sit in LDS, beyond it in a row of device memory per workgroup;
 * *counters_in_lds = n_nodes <= lds_nodes.  list_cut: when the taxonomy is attached a key's list of more holders than this is
 * folded by a whole wave instead of one lane (classify's list_cut).  SPSP_ERR_ARG: n_nodes outside 1 .. 1 048 576. */
int spsp_taxonomy_plan_host(uint32_t n_nodes, uint32_t* small_hits, uint32_t* lds_nodes, uint32_t* counters_in_lds, uint32_t* list_cut);
/* Attaches a taxonomy to the index spsp_classify_index_device built on the context: checks the arrays
 * (spsp_taxonomy_check_host), uploads parent, size and ref_node, and one launch writes node(x) for every distinct key from the
 * 16-bit holder lists -- a lane per key, a list of more than list_cut holders by a whole wave; the fold is the smallest and the
 * largest ref_node of the list and one climb, because in preorder the lca of a set is the lca of its two extremes.  The taxonomy
 * lives with the index and ends when the index ends (a prevalence, select, accumulation, groups or index call); a second attach
 * replaces it.  The counters of a depth pass begun on the index are not touched.  *key_nodes_out (may be NULL) receives the device
 * address of a context-owned uint32 array parallel to the index's key arrays (entry e at [e - h_sk_off[0]]): node(x) of that
 * entry's key, valid until the next attach or index call.  One host wait.  SPSP_ERR_ARG: no index on the context, n_ref not the
 * index's, arrays the check refuses. */
int spsp_taxonomy_index_device(spsp_ctx* ctx, const uint32_t* parent, uint32_t n_nodes, const uint32_t* ref_node, uint32_t n_ref,
                               const void** key_nodes_out /* may be NULL */);
/* Assigns one batch of records, given exactly as spsp_classify_device takes them (any device arrays, distinct keys per record in
 * any order, n_records bounded by the entry extent).  records: n_records (length is not touched).  Any number of batches on one
 * index; one host wait per call.  Launches: classify's probe pass, unchanged (a record's hit keys route it; its work is ignored),
 * a routing pass, and the two forms (spsp_taxonomy_plan_host).  SPSP_ERR_ARG (records zeroed): no index or no taxonomy on the
 * context, d_q_kmer_hi against the index's k, min_keys, num or den out of range, decreasing offsets; SPSP_ERR_OVERFLOW: an extent
 * above 0xfffffff0. */
int spsp_taxonomy_device(spsp_ctx* ctx, const void* d_q_minimizer, const void* d_q_kmer_lo, const void* d_q_kmer_hi /* NULL if k <= 32 */,
                         const uint64_t* h_rec_off /* n_records + 1 */, uint32_t n_records, uint32_t min_keys, uint32_t num, uint32_t den,
                         spsp_taxonomy_record* records /* n_records */);
/* While the context's timing is on a taxonomy call records events between its launches; this reads the milliseconds added up since
 * the last read and clears them: ms[0] the probe pass, ms[1] the routing pass, ms[2] the wave form, ms[3] the workgroup form. */
int spsp_taxonomy_stage_ms(spsp_ctx* ctx, double* ms /* 4 */);
/* The text of <prefix>_taxonomy.csv.gz: "record,name,length,keys,hit_keys,taxon,depth,lineage,score,clade,direct,f_clade,winners"
 * and one line per record.  taxon = the node's number, depth = its depth, lineage = the names from below the root down to it joined
 * by ';' (empty for the root); an unclassified record has an empty taxon, depth and lineage.  f_clade = clade / keys as
 * %.<precision>g (0 when keys == 0 or unclassified; it decides nothing).  node_names: n_nodes names.  A row that contradicts itself
 * is SPSP_ERR_ARG, the message naming the record: hit_keys > keys, clade > hit_keys, direct > clade, score > hit_keys, node >=
 * n_nodes and not SPSP_TAXONOMY_NONE, node not anc of start, winners == 0 with hit_keys > 0.  A tree spsp_taxonomy_check_host
 * refuses is refused here.  *text is released with spsp_free(). */
int spsp_taxonomy_csv_host(const spsp_taxonomy_record* records, uint64_t n_records, const char* const* record_names, const uint32_t* parent,
                           uint32_t n_nodes, const char* const* node_names, int precision, char** text, uint64_t* len);
/* The text of <prefix>_taxonomy_report.csv.gz (the columns of a Kraken report):
 * "taxon,depth,name,lineage,references,records_clade,records_direct,bases_clade,bases_direct" and one line per node in preorder --
 * references = the references that sit at the node itself, records_direct and bases_direct = the records called at the node and
 * their lengths, _clade = the same over the node's subtree -- closed by one line ",,unclassified,,0,n,n,bases,bases".  The same
 * refusals. */
int spsp_taxonomy_report_csv_host(const spsp_taxonomy_record* records, uint64_t n_records, const uint32_t* parent, uint32_t n_nodes,
                                  const char* const* node_names, const uint32_t* ref_node, uint32_t n_ref, char** text, uint64_t* len);
/* The whole-file driver: spsp_classify_files' road (the same code: loading and `rate` refusals, the second context, one scan,
 * batches of 65 535 records) with the lineage file read and parsed first, the taxonomy attached behind the index, and every batch
 * handed to spsp_taxonomy_device.  Writes <out_prefix>_taxonomy.csv.gz and <out_prefix>_taxonomy_report.csv.gz (gzip level 1);
 * nothing on any failure.  With chatter one line of totals: records, classified, and the share of the classified at depth 0.
 * records (may be NULL) receives a copy released with spsp_free(); *n_records (may be NULL) their number. */
int spsp_taxonomy_files(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                        uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                        spsp_taxonomy_record** records /* may be NULL; spsp_free */, uint64_t* n_records /* may be NULL */);

/* ------------------------------------------------------------- extract ---- */
/* The records a record pass calls, written out again as FASTA / FASTQ (not in the reference): what follows a classify or taxonomy
 * call -- host depletion, the reads of one species or clade, the contigs a contaminant index claims.
 * TEXT T of n bytes.  It is FASTQ when n > 0 and T[0] == '@', else FASTA: how every sketch path tells them apart.
 * FASTA RECORDS.  A line begins at byte 0 and behind every '\n'.  Line 0, and every line whose first byte is '>' or 0xFF, begins a
 * record (the ingest's rule for a dropped line, to the letter: line 0 is a header whatever it holds).  With b_0 < b_1 < ... the
 * bytes that begin a record, record r is the byte range [b_r, b_(r+1)) and b_(n_rec) = n.  Every byte of the text lies in exactly
 * one record: the records concatenated are the text.  n_rec is what spsp_fasta_clean_device reports for the same text; the empty
 * text is one empty record.
 * FASTQ RECORDS.  content_end is behind the last byte that is neither '\n' nor '\r'; the blank tail is what follows it.  The lines
 * of T[0, content_end) are counted and nothing else is checked (the file drivers have ingested, and so validated, the text first):
 * a line count that is not a multiple of four is SPSP_ERR_FORMAT.  Record r is lines 4r .. 4r+3: from the first byte of line 4r to
 * one past the '\n' that ends line 4r+3.  For the last record that '\n' is the first one of the blank tail; where the tail has
 * none the record ends at content_end.  The rest of the blank tail belongs to no record.  A quality line that begins with '@' or
 * '>' begins nothing.  One content of 4r + 3 lines is a whole record all the same, as the ingest has it: when something follows
 * the blank tail's first newline, the last record's quality line is the empty line behind that newline, and the record ends behind
 * the tail's second newline (at n where there is none).  n_rec is what spsp_fastq_clean_device reports.
 * begin[0 .. n_rec]: record r is [begin[r], begin[r + 1]) in both formats.
 * OUTPUT.  keep[r] is one byte per record.  The output is the concatenation, in record order, of the byte ranges of the records
 * with keep[r] != 0, verbatim: '\r' bytes, lower-case bases, wrapped FASTA lines, header comments and quality strings pass through
 * unchanged.  One exception: a kept range that is not empty and whose last byte is not '\n' gets one '\n' appended; only the last
 * record of a text can be such a range.  So every output is a well-formed file and outputs can be concatenated.  n_kept = the
 * records with keep[r] != 0, n_out = the output's bytes.  Extents are 64-bit; the text is bounded by what the ingest accepts.
 * WHICH RECORDS.  A word `what` and the rows of a pass make the flags, on the host, without floating point.
 *   classify rows:  matched: listed >= 1.  unmatched: listed == 0.  best=<j>: the rank-1 match is reference <j>.
 *                   listed=<j>: reference <j> is among the listed matches.  <j> is the 0-based list position.
 *   taxonomy rows:  classified: node != SPSP_TAXONOMY_NONE.  unclassified: node == SPSP_TAXONOMY_NONE.  taxon=<t>: node == t.
 *                   clade=<t>: t <= node < t + size[t], the preorder range test.  <t> is the number the taxonomy CSV prints.
 * Anything else is SPSP_ERR_ARG naming the word; so are <j> >= n_ref, <t> >= n_nodes, a classify word with taxonomy rows and the
 * reverse.  Numbers are decimal digits only. */
/* The two constants the kernels cut at (either pointer may be NULL): the bytes of the text one workgroup of the starts pass reads,
 * and the bytes of the output one workgroup of the copy owns. */
int spsp_extract_plan_host(uint32_t* tile_bytes, uint32_t* stretch_bytes);
/* The rule as plain loops on the host.  *begin: n_rec + 1 offsets, released with spsp_free().  SPSP_ERR_FORMAT: a FASTQ content
 * whose lines are not a multiple of four. */
int spsp_records_extents_host(const uint8_t* text, uint64_t n_text, uint64_t** begin /* spsp_free */, uint32_t* n_rec);
/* begin: n_rec + 1 offsets that do not decrease and end inside the text (SPSP_ERR_ARG otherwise) -- the rule's, or any ranges of
 * the caller's own: then, here and on the device, only the LAST range is looked at for the newline rule.  *out: spsp_free(). */
int spsp_records_extract_host(const uint8_t* text, uint64_t n_text, const uint64_t* begin, uint32_t n_rec, const uint8_t* keep /* n_rec */,
                              uint8_t** out /* spsp_free */, uint64_t* n_out, uint64_t* n_kept);
/* The flags of a word.  hits: n_records * top, as spsp_classify_device fills them; size: the tree's subtree sizes (n_nodes), as
 * spsp_taxonomy_lineages_host hands them out.  SPSP_ERR_ARG as the rule says, and for a record that lists more than top matches. */
int spsp_extract_flags_classify_host(const char* what, const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records,
                                     uint32_t top, uint32_t n_ref, uint8_t* keep /* n_records */);
int spsp_extract_flags_taxonomy_host(const char* what, const spsp_taxonomy_record* records, uint64_t n_records, const uint32_t* size, uint32_t n_nodes,
                                     uint8_t* keep /* n_records */);
/* Only the refusals of a word: taxonomy != 0 asks for a taxonomy word; limit is n_ref or n_nodes (0xffffffff: not known yet). */
int spsp_extract_word_check_host(const char* what, int taxonomy, uint32_t limit);
/* The records' starts of a text in HBM (16-byte aligned, as the ingest takes it): *d_begin is a context-owned array of n_rec + 1
 * uint64, valid until the next extents call or the next extract call that makes its own starts.  Launches: one workgroup that
 * finds the text's kind, its content end and its last record's end; per 4 KiB tile a count (FASTA: record starts, FASTQ:
 * newlines); one composing scan; per tile the write.  It reads the text alone, not the ingest's outputs.  One host wait, for n_rec.
 * SPSP_ERR_FORMAT as above. */
int spsp_records_extents_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, void** d_begin, uint32_t* n_rec);
/* The kept records of a text in HBM, back to back in a context-owned buffer (*d_out, valid until the next extract call on the
 * context; spsp_copy_to_host brings it back).  d_begin: the starts on the device, n_rec + 1 of them -- the array of an extents
 * call may be handed back in -- or NULL: they are made here for n_rec records, without a wait of their own, and a text that holds
 * another number of records is SPSP_ERR_ARG.  h_keep: n_rec bytes on the host.  Launches: per 2 048 records the kept bytes and
 * the runs of consecutive kept records, the same scan, the run table (source start, output start); then the copy, balanced by
 * output bytes: a workgroup owns spsp_extract_plan_host's stretch of the output, finds the runs that cross it by binary search, and
 * writes aligned 16-byte stores -- from two aligned loads and a byte shift inside a run, byte by byte across runs.  One host wait,
 * for n_out.  SPSP_ERR_ARG also for starts that decrease or leave the text (nothing is read or written outside the buffers). */
int spsp_records_extract_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, const void* d_begin /* NULL: made here */, uint32_t n_rec,
                                const uint8_t* h_keep /* n_rec */, void** d_out, uint64_t* n_out, uint64_t* n_kept);
/* While the context's timing is on an extract call records events between its launches; this reads the milliseconds added up since
 * the last read and clears them: ms[0] the starts (0 when they were handed in), ms[1] the offsets and the run table, ms[2] the copy. */
int spsp_extract_stage_ms(spsp_ctx* ctx, double* ms /* 3: starts, offsets, copy */);
/* The whole-file drivers with an extraction: the arguments of spsp_classify_files / spsp_taxonomy_files, the same code and the
 * same CSVs byte for byte, plus the word.  Behind the records file's last batch the flags are made from the rows and the kept
 * records are extracted on the second context, where the text still sits; only the kept bytes come back.  Writes
 * <out_prefix>_extract.fa or _extract.fq (by the text's kind), gzip level 1 with ".gz" appended when gz != 0.  A word that is
 * refused is refused before any file is read (a taxonomy word's node: once the lineage file is).  *n_kept, *bytes_out (may be
 * NULL): the records kept and the bytes of the output before compression. */
int spsp_classify_files_extract(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys,
                                uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                                spsp_classify_record** records /* may be NULL; spsp_free */, spsp_classify_hit** hits /* may be NULL; spsp_free */,
                                uint64_t* n_records /* may be NULL */, const char* what, int gz, uint64_t* n_kept, uint64_t* bytes_out);
int spsp_taxonomy_files_extract(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                                uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                                spsp_taxonomy_record** records /* may be NULL; spsp_free */, uint64_t* n_records /* may be NULL */, const char* what,
                                int gz, uint64_t* n_kept, uint64_t* bytes_out);

/* ------------------------------------------------------- paired records ---- */
/* Mate pairs classified and extracted as one record (not in the reference): Illumina data comes as two files, and record p of one
 * and record p of the other are the two ends of one fragment -- the unit of evidence and of output.
 * PAIR.  Pair p is record p of the records file (mate 1) together with record p of the mates file (mate 2).  The two files may be
 * of different kinds (FASTA and FASTQ) and either may be gzip or plain.  Two files with different record counts are
 * SPSP_ERR_FORMAT, and the error text gives both counts.
 * KEYS.  Q_p = Q_p^1 u Q_p^2, where Q^i is exactly the record key set classify defines: spsp_sketch_keys_device over the one
 * record, abundance 1, at the index's threshold.  A key present in both mates counts once (the mates of a short fragment overlap,
 * and canonical k-mers make the reverse-complement mate produce the same keys).  keys = |Q_p|.  A mate without keys (shorter than
 * k, or with no selected minimizer) contributes nothing; a pair whose mates both have none has keys = 0, as a record has.
 * LENGTH.  The bases of mate 1 plus the bases of mate 2.
 * FROM THERE ON A PAIR IS A RECORD.  Every threshold, tie rule, CSV column and report of classify and taxonomy applies to Q_p to
 * the letter; the CSVs keep their columns, and `record` is the pair's number.
 * NAME.  The pair's common name: the first whitespace-delimited word of mate 1's header with one trailing "/1" removed if present.
 * Mate 2's first word with one trailing "/2" removed must equal it, byte for byte; a pair whose two names differ is
 * SPSP_ERR_FORMAT, and the error text gives the pair's number and both names (files that have slipped out of step must not
 * produce a CSV).  Both checks come before anything is computed.
 * EXTRACT.  The flag functions run on the pairs' rows; the one flag vector cuts both texts, so <out_prefix>_extract_1.fa|fq[.gz]
 * and <out_prefix>_extract_2.fa|fq[.gz] (each by its own text's kind) hold the same pairs in the same order: a mate is never
 * kept without the other.
 * Out of scope: depth and profile over fragments (they stay per record), interleaved single-file pairs, more than two mates. */
/* The naming rule on the host.  names1 / names2: n first words each, as the headers hold them.  *bad = n and SPSP_OK, or the first
 * pair whose names differ and SPSP_ERR_FORMAT.  common (may be NULL): the n common names, each ended by a 0 byte, back to back;
 * spsp_free(). */
int spsp_pairs_names_host(const char* const* names1, const char* const* names2, uint64_t n, char** common /* may be NULL; spsp_free */, uint64_t* bad);
/* The constants the union's kernels cut at (either pointer may be NULL): the lanes of a workgroup (a lane per key), and the
 * entries of B per count of the scan. */
int spsp_union_plan_host(uint32_t* threads, uint32_t* tile);
/* Per record r of n_records the union of A_r = entries [h_a_off[r], h_a_off[r + 1]) of the arrays A and B_r likewise: each side
 * per record distinct and strictly ascending by (minimizer, kmer_hi, kmer_lo), which is what the sorted form of
 * spsp_sketch_keys_device returns.  The inputs are the caller's (the key arrays of two other contexts, say), only read, and their
 * offsets need not start at 0; kmer_hi is NULL on both sides iff k <= 32.  The output arrays are the context's, valid until its
 * next union call: per record the union, distinct and strictly ascending -- a function of the two sets alone, for any call that
 * wants sorted keys; h_off (n_records + 1, from 0) are its offsets.  A lane per key, never per record: a lane's trip count grows
 * with a record's keys only through the logarithm of a binary search.  Launches: the flags (per entry of B: its place in A_r and
 * whether A_r holds it; per entry of either side: its order), one scan over the tiles' counts, the offsets, the write.  One host
 * wait, at the end.  Refused, in this order: k outside 1..63 (ARG), more than 0xfffffff0 records (OVERFLOW), offsets that decrease
 * (ARG), more than 0xfffffff0 keys on both sides together (OVERFLOW), a NULL key array, kmer_hi against k (ARG), and, behind the
 * wait, a record whose keys are not strictly ascending (ARG; the text names the side and the record).  A refused call hands out
 * NULL arrays and offsets that are all 0. */
int spsp_records_union_device(spsp_ctx* ctx, uint32_t k, const void* d_a_min, const void* d_a_lo, const void* d_a_hi /* NULL if k <= 32 */,
                              const uint64_t* h_a_off /* n + 1 */, const void* d_b_min, const void* d_b_lo, const void* d_b_hi,
                              const uint64_t* h_b_off /* n + 1 */, uint32_t n_records, void** d_min, void** d_lo, void** d_hi, uint64_t* h_off /* n + 1, from 0 */);
/* While the context's timing is on a union call records events between its launches; this reads the milliseconds added up since
 * the last read and clears them. */
int spsp_union_stage_ms(spsp_ctx* ctx, double* ms /* 4: flags, scan, offsets, write */);
/* The whole-file drivers over pairs: the arguments of spsp_classify_files_extract / spsp_taxonomy_files_extract with the mates
 * file behind the records file, and what == NULL meaning no extraction.  Each file is ingested and scanned once on a side context
 * of its own; per batch of at most 65 535 pairs the two key extractions run on the two sides' streams, one union on ctx makes the
 * pairs' keys, and the unchanged spsp_classify_device / spsp_taxonomy_device work of a batch follows.  *n_records: the pairs;
 * *n_kept: the pairs kept; *bytes_out: the bytes of both outputs before compression. */
int spsp_classify_files_paired(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* mates_path, uint32_t top,
                               uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                               const char* what /* NULL: no extraction */, int gz, spsp_classify_record** records /* may be NULL; spsp_free */,
                               spsp_classify_hit** hits /* may be NULL; spsp_free */, uint64_t* n_records /* may be NULL */, uint64_t* n_kept,
                               uint64_t* bytes_out);
int spsp_taxonomy_files_paired(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* mates_path,
                               const char* lineages_path, uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter,
                               double rate, const char* what /* NULL: no extraction */, int gz, spsp_taxonomy_record** records /* may be NULL; spsp_free */,
                               uint64_t* n_records /* may be NULL */, uint64_t* n_kept, uint64_t* bytes_out);

/* --------------------------------------------------------------- split ---- */
/* Every record written to the file of its reference or taxon, all files in one pass (not in the reference): binning a read set or
 * the contigs of an assembly, which the extraction does one subset -- and one run -- at a time.
 * RECORDS.  The text's kind, the records and begin[0 .. n_rec] are exactly what the extract section defines.
 * BINS.  bin[r] is one uint32 per record.  SPSP_SPLIT_DROP: the record is not written.  Every other value must be < n_bins, else
 * SPSP_ERR_ARG naming the first such record.  1 <= n_bins <= SPSP_SPLIT_MAX_BINS = 2^24 (a tree has at most 1 048 576 nodes and a
 * list 65 535 references, so either count + 1 fits); another n_bins is SPSP_ERR_ARG.
 * OUTPUT.  The slices of bin 0, 1, ..., n_bins - 1 follow one another.  Within a bin the byte ranges of its records come verbatim
 * and in record order: the split is stable.  The extract section's one exception holds: a range that is not empty and whose last
 * byte is not '\n' gets one '\n' appended, and only the text's last range can be such a range -- but that range can now land
 * anywhere in the output, and its bin is one byte longer than its source bytes.  bin_off[0 .. n_bins] are the bins' byte offsets
 * in the output, from 0; an empty bin repeats the offset; bin_off[n_bins] = n_out.  bin_records[b] = the records with bin[r] == b,
 * empty ranges included (as n_kept counts flagged records).  With a caller's own begin[] only the last range is looked at for the
 * newline, as in extract.  So every bin's slice is a well-formed file.
 * WHICH BIN.  A word `what` and the rows of a pass make the bins, on the host, in integers only.
 *   classify rows:  best: n_bins = n_ref + 1; bin = the rank-1 match's list position; a record with listed == 0 goes to bin n_ref,
 *                   "unmatched".
 *   taxonomy rows:  taxon: n_bins = n_nodes + 1; bin = node; SPSP_TAXONOMY_NONE goes to bin n_nodes, "unclassified".
 *                   depth=<d>, 1 <= d <= 32 in decimal digits (the depths spsp_taxonomy_lineages_host hands out and the taxonomy
 *                   CSV prints): a record whose node lies at depth >= d goes to that node's ancestor at depth d -- one file per
 *                   species when the lineage file's d-th name is the species; a record called above depth d keeps its own node
 *                   (nothing is lost, nothing is pushed down); unclassified records as in taxon.
 * Anything else is SPSP_ERR_ARG naming the word; so are a classify word with taxonomy rows and the reverse, d == 0 and d > 32. */
#define SPSP_SPLIT_DROP 0xffffffffu
#define SPSP_SPLIT_MAX_BINS 16777216u
/* What the kernels cut at (any pointer may be NULL): the bytes of the output one workgroup of the copy owns (the extraction's
 * stretch), the records -- and the sorted runs -- per workgroup of the run table's and the offsets' passes, the pairs per workgroup
 * of the sort, and SPSP_SPLIT_MAX_BINS. */
int spsp_split_plan_host(uint32_t* stretch_bytes, uint32_t* record_tile, uint32_t* sort_tile, uint32_t* max_bins);
/* The rule as plain loops on the host.  begin: as spsp_records_extract_host takes it.  *out, *bin_off (n_bins + 1) and
 * *bin_records (n_bins) are released with spsp_free(). */
int spsp_records_split_host(const uint8_t* text, uint64_t n_text, const uint64_t* begin, uint32_t n_rec, const uint32_t* bin /* n_rec */, uint32_t n_bins,
                            uint8_t** out /* spsp_free */, uint64_t* n_out, uint64_t** bin_off /* spsp_free */, uint64_t** bin_records /* spsp_free */);
/* The bins of a word.  hits: n_records * top; parent, depth: the tree's arrays (n_nodes), as spsp_taxonomy_lineages_host hands
 * them out.  SPSP_ERR_ARG as the rule says, for a record that lists more than top matches, and for a reference or node out of range. */
int spsp_split_bins_classify_host(const char* what, const spsp_classify_record* records, const spsp_classify_hit* hits, uint64_t n_records, uint32_t top,
                                  uint32_t n_ref, uint32_t* bin /* n_records */, uint32_t* n_bins);
int spsp_split_bins_taxonomy_host(const char* what, const spsp_taxonomy_record* records, uint64_t n_records, const uint32_t* parent, const uint32_t* depth,
                                  uint32_t n_nodes, uint32_t* bin /* n_records */, uint32_t* n_bins);
/* Only the refusals of a word: taxonomy != 0 asks for a taxonomy word. */
int spsp_split_word_check_host(const char* what, int taxonomy);
/* The text of <prefix>_split.csv.gz: "bin,name,records,bytes,file" and one line per bin with records, in bin order -- with
 * bin_off_mates, "bin,name,records,bytes_1,file_1,bytes_2,file_2".  bin = the bin's number, or last_name for bin n_bins - 1;
 * name = names[b], or last_name; file = <file_prefix>_split_<bin><suffix>, paired <file_prefix>_split_<bin>_1<suffix> and
 * <file_prefix>_split_<bin>_2<suffix_mates>.  names: n_bins - 1.  *text is released with spsp_free(). */
int spsp_split_csv_host(const char* file_prefix, const char* const* names /* n_bins - 1 */, const char* last_name, uint32_t n_bins,
                        const uint64_t* bin_records /* n_bins */, const uint64_t* bin_off /* n_bins + 1 */, const char* suffix,
                        const uint64_t* bin_off_mates /* NULL: not paired */, const char* suffix_mates, char** text, uint64_t* len);
/* The bins' slices of a text in HBM, back to back in the context's output buffer (*d_out: the extraction's buffer, valid until the
 * next split or extract call on the context).  The conventions of spsp_records_extract_device: a 16-byte aligned text; d_begin NULL
 * = the starts are made here for n_rec records, without a wait of their own, and a text that holds another number is SPSP_ERR_ARG;
 * starts that decrease or leave the text are SPSP_ERR_ARG, and nothing is read or written outside the buffers.  h_bin: n_rec words
 * on the host; h_bin_off: n_bins + 1, h_bin_records: n_bins, the caller's (zero on a refusal).  Launches: the starts; per 2 048
 * records the kept bytes and the RUNS -- consecutive records of one bin, neither dropped nor empty -- then the extraction's scan and
 * the run table; the stable 8-bit LSD radix sort of the runs by bin (spsp_sketch_build_device's), one pass per byte of n_bins - 1,
 * none for n_bins == 1; a 64-bit scan of the sorted runs' lengths and a lane per bin for bin_off; then the extraction's copy over
 * runs whose sources lie anywhere in the text, with the appended newline anywhere in the output.  One host wait, at the end. */
int spsp_records_split_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, const void* d_begin /* NULL: made here */, uint32_t n_rec,
                              const uint32_t* h_bin /* n_rec */, uint32_t n_bins, void** d_out, uint64_t* n_out, uint64_t* h_bin_off /* n_bins + 1 */,
                              uint64_t* h_bin_records /* n_bins */);
/* While the context's timing is on a split call records events between its launches; this reads the milliseconds added up since
 * the last read and clears them. */
int spsp_split_stage_ms(spsp_ctx* ctx, double* ms /* 5: starts, runs, order, offsets, copy */);
/* The whole-file drivers with a split: the arguments of spsp_classify_files_paired / spsp_taxonomy_files_paired (mates_path may be
 * NULL) with the split word in the place of the extraction's, the same road and the same CSVs byte for byte.  Behind a file's last
 * batch the bins are made from the rows, the split runs on the second context, where the text still sits, and the output comes back
 * once and is cut at bin_off on the host.  With mates_path one bin vector, made from the pairs' rows, cuts both texts.  Writes one
 * file per bin with records, <out_prefix>_split_<b>.fa|fq[.gz] -- <b> the reference's list position or the node's number, the last
 * bin <out_prefix>_split_unmatched.* or _split_unclassified.* -- paired <out_prefix>_split_<b>_1.* and _2.*, each by its own text's
 * kind; gzip level 1 when gz != 0; and always <out_prefix>_split.csv.gz (spsp_split_csv_host).  Nothing on any failure; a refused
 * word is refused before any file is read.  *n_bins_written, *bytes_out (may be NULL): the bins with files, and the bytes of all
 * slices before compression. */
int spsp_classify_files_split(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* mates_path /* may be NULL */,
                              uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                              const char* what, int gz, spsp_classify_record** records /* may be NULL; spsp_free */,
                              spsp_classify_hit** hits /* may be NULL; spsp_free */, uint64_t* n_records /* may be NULL */, uint64_t* n_bins_written,
                              uint64_t* bytes_out);
int spsp_taxonomy_files_split(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* mates_path /* may be NULL */,
                              const char* lineages_path, uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter,
                              double rate, const char* what, int gz, spsp_taxonomy_record** records /* may be NULL; spsp_free */,
                              uint64_t* n_records /* may be NULL */, uint64_t* n_bins_written, uint64_t* bytes_out);

/* ------------------------------------------------------------- windows ---- */
/* A long record called stretch by stretch (not in the reference): every record is cut into overlapping windows on the device,
 * between the ingest and the scan; the windows run as records through the unchanged scan, key extraction, classify and taxonomy
 * kernels; the answer comes back along the record as SEGMENTS and one MOSAIC line per record.
 * BASES.  A record r has L bases: the bases the ingest keeps (bytes outside ACGTacgt are deleted); `length` and every position
 * below count what is left.  Positions in the raw text, where it holds Ns, are made from them afterwards: "raw coordinates" below.
 * WINDOWS.  A width W with k <= W <= 0x7fffffff (else SPSP_ERR_ARG); the step is S = W - (k - 1).
 *   n_win(r) = max(1, ceil((L - k + 1) / S)): a record of at most W bases is one window, a record shorter than k one window
 *   without keys, an empty record one empty window.
 *   Window i of r holds the bases [i S, min(i S + W, L)): every window but a record's last has exactly W bases, and the last has
 *   at least k when L >= k.  Consecutive windows overlap by k - 1 bases, so every k-mer of the record lies in exactly one window.
 *   Window i OWNS the stretch [i S, (i + 1) S), a record's last window up to L: the owned stretches tile [0, L).
 *   The windows of all records follow one another in record order; first_win[0 .. n_rec] is each record's first window and
 *   n_windows = first_win[n_rec].  More than 0xfffffff0 windows is SPSP_ERR_OVERFLOW (the scan numbers records in 32 bits).
 * KEY SET.  A window's key set is what spsp_sketch_keys_device returns for the genome made of that window's bases alone (the uint8
 *   count rule included): classify's Q_r with the window in the record's place.  Every threshold and tie rule of classify or
 *   taxonomy applies to the window to the letter.
 * CALL.  A window's call is the bin spsp_split_bins_classify_host("best") gives its row -- with taxonomy rows the bin of
 *   spsp_split_bins_taxonomy_host("taxon" | "depth=<d>").  The last bin (n_ref, or n_nodes) means no call.
 * SEGMENT.  A maximal run of consecutive windows of ONE record with the same call.  begin = the first window's owned start, end =
 *   the last window's owned end; the segments of a record tile [0, L).  A segment carries the sums of its windows' keys, hit_keys
 *   and support (the rank-1 `shared` of classify rows, the taxon's clade keys of taxonomy rows; 0 where there is no call).
 * MOSAIC.  One line per record: length, windows, segments, called_windows (windows with a call), calls (the distinct calls other
 *   than "none"); major = the call other than "none" with the most owned bases, among equals the lower number, with its windows
 *   and owned bases; second likewise among the other calls; SPSP_WINDOWS_ABSENT (and zeros) where there is no such call; the sums
 *   of keys and hit_keys.  Integers decide everything; the one printed ratio, f_major = major_bases / length (0 for an empty
 *   record), decides nothing. */
#define SPSP_WINDOWS_ABSENT 0xffffffffu
#define SPSP_WINDOWS_MAX_WIDTH 0x7fffffffu
typedef struct spsp_segment_row {
    uint64_t begin, end;             /* the owned stretch [begin, end) in the record's bases */
    uint64_t keys, hit_keys, support;
    uint32_t record, segment;        /* the record, and the segment's number within it */
    uint32_t windows, call;          /* call == n_bins - 1: none */
} spsp_segment_row;                  /* 56 bytes */
typedef struct spsp_mosaic_row {
    uint64_t length, major_bases, second_bases, keys, hit_keys;
    uint32_t windows, segments, called_windows, calls;
    uint32_t major, major_windows, second, second_windows;
} spsp_mosaic_row;                   /* 72 bytes */
/* What the kernels cut at (any pointer may be NULL): the output bases one workgroup of the copy owns in the ASCII form and in the
 * packed form (16 KiB of output either way), and the records per workgroup of the counting pass. */
int spsp_windows_plan_host(uint32_t* stretch_bases, uint32_t* stretch_bases_packed, uint32_t* record_tile);
/* The counting rule from offsets alone.  first_win: n_rec + 1, the caller's; *win_off: n_windows + 1 base offsets of the windows
 * in the expanded text, spsp_free(); *n_bases = win_off[n_windows].  SPSP_ERR_ARG for a width outside k .. 0x7fffffff and for
 * offsets that decrease, SPSP_ERR_OVERFLOW as the rule says (nothing is allocated then). */
int spsp_records_windows_host(const uint64_t* rec_off /* n_rec + 1 */, uint32_t n_rec, uint32_t k, uint64_t window, uint32_t* first_win /* n_rec + 1 */,
                              uint64_t** win_off /* spsp_free */, uint64_t* n_windows, uint64_t* n_bases);
/* The expansion as plain loops over ASCII bases: the windows' bases back to back in *out (spsp_free), the rest as above. */
int spsp_windows_expand_host(const uint8_t* bases, const uint64_t* rec_off /* n_rec + 1 */, uint32_t n_rec, uint32_t k, uint64_t window, uint8_t** out /* spsp_free */,
                             uint64_t* n_out, uint32_t* first_win /* n_rec + 1 */, uint64_t** win_off /* spsp_free */, uint64_t* n_windows);
/* Segments and mosaic rows from the windows' calls and addends (n_windows = first_win[n_rec] of each).  *segments: spsp_free();
 * mosaic: n_rec rows, the caller's.  Rows that contradict themselves are SPSP_ERR_ARG naming the record: a call >= n_bins, or a
 * first_win that is not what the rule makes of the offsets. */
int spsp_windows_segments_host(const uint32_t* call, const uint32_t* keys, const uint32_t* hit_keys, const uint32_t* support, const uint32_t* first_win /* n_rec + 1 */,
                               const uint64_t* rec_off /* n_rec + 1 */, uint32_t n_rec, uint32_t k, uint64_t window, uint32_t n_bins,
                               spsp_segment_row** segments /* spsp_free */, uint64_t* n_segments, spsp_mosaic_row* mosaic /* n_rec */);
/* The texts of <prefix>_segments.csv.gz -- "record,name,segment,begin,end,windows,call,call_name,keys,hit_keys,support" -- and of
 * <prefix>_mosaic.csv.gz -- "record,name,length,windows,segments,called_windows,calls,major,major_name,major_windows,major_bases,
 * f_major,second,second_name,second_windows,second_bases,keys,hit_keys".  call_names: n_bins - 1 (the references' names or the
 * nodes'); the last bin prints as last_name ("unmatched", "unclassified") in both columns; an absent major or second prints as
 * empty fields.  *text is released with spsp_free(). */
int spsp_segments_csv_host(const spsp_segment_row* segments, uint64_t n_segments, const char* const* record_names, uint32_t n_rec, const char* const* call_names,
                           const char* last_name, uint32_t n_bins, char** text, uint64_t* len);
int spsp_mosaic_csv_host(const spsp_mosaic_row* mosaic, uint32_t n_rec, const char* const* record_names, const char* const* call_names, const char* last_name,
                         uint32_t n_bins, int precision, char** text, uint64_t* len);
/* Only the refusals of a call word (best; with a taxonomy: taxon, depth=<d>): the split's words. */
int spsp_windows_word_check_host(const char* what, int taxonomy);
/* The expansion on the device.  d_bases: the cleaned bases of a text in HBM in either form the ingest writes -- ASCII (packed == 0)
 * or the 2-bit words of SPSP_SCAN_PACKED_INPUT (16 bases per dword, first base in bits 31:30), 16-byte aligned, the packed form
 * with its readable bytes behind; d_rec_off: the records' n_rec + 1 base offsets on the device.  *d_out: the windows' bases back to
 * back in the same form, in a buffer the context owns (valid until its next windows call): zero behind the last base up to a whole
 * stretch, 256 zero bytes behind that, 16-byte aligned -- what a scan takes.  *d_win_off: the windows' n_windows + 1 base offsets
 * on the device, the context's as well; h_first_win: n_rec + 1, the caller's.  Launches: per spsp_windows_plan_host's record tile
 * the windows and the expanded bases; one 64-bit scan; ONE host wait, for the counts; per tile the records' first windows and
 * output starts; per window its offset and its source; then the copy, balanced by OUTPUT: a workgroup owns a stretch of whole
 * 16-byte stores, finds the windows that cross it by binary search over the new offsets, and writes every store whole.  ASCII: two
 * aligned loads and a byte shift inside a window, byte by byte across windows.  Packed: per output dword a funnel shift of two
 * source dwords by twice the source's offset in its dword, looped where a dword holds bases of several windows.  Nothing is read
 * or written outside the buffers; no store is shared between workgroups.  Refused: the width (ARG), offsets that decrease or leave
 * the bases (ARG), too many windows (OVERFLOW). */
int spsp_records_windows_device(spsp_ctx* ctx, const void* d_bases, uint64_t n_bases, const void* d_rec_off, uint32_t n_rec, uint32_t k, uint64_t window, int packed,
                                void** d_out, uint64_t* n_out, void** d_win_off, uint32_t* h_first_win /* n_rec + 1 */, uint64_t* n_windows);
/* While the context's timing is on a windows call records events between its launches; this reads the milliseconds added up since
 * the last read and clears them. */
int spsp_windows_stage_ms(spsp_ctx* ctx, double* ms /* 3: count, offsets, copy */);
/* The whole-file driver over windows: the arguments of spsp_classify_files plus the width and the call word ("best").  Behind the
 * ingest and in front of the scan the expansion runs on the second context; the scan, the key extraction and spsp_classify_device
 * then see windows as records, in batches of at most 65 535 windows; the header count is still held against the real records.
 * Writes <out_prefix>_segments.csv.gz and <out_prefix>_mosaic.csv.gz in the place of the per-record CSVs (the per-record call of a
 * windowed run is the mosaic line); nothing on any failure; a refused word or width is refused before any file is read.  Handed
 * out (each may be NULL; spsp_free): the windows' rows and hits, first_win (n_records + 1), the segments and the mosaic rows. */
int spsp_classify_files_windows(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys,
                                uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window, const char* what,
                                spsp_classify_record** rows, spsp_classify_hit** hits, uint64_t* n_windows, uint32_t** first_win, uint64_t* n_records,
                                spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic);
int spsp_taxonomy_files_windows(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                                uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window,
                                const char* what, spsp_taxonomy_record** rows, uint64_t* n_windows, uint32_t** first_win, uint64_t* n_records,
                                spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic);

/* ------------------------------------------------- segments as sequence ---- */
/* What follows the windows (not in the reference): single stray windows absorbed into the stretch around them, and chosen
 * segments written out as FASTA from the cleaned bases the side context still holds.  Coordinates count kept BASES, as above.
 * SMOOTHING.  q, an integer 0 .. 0x7fffffff; 0 changes nothing.  The RUNS of a record are the maximal runs of equal calls among
 *   its windows (the segments of the unsmoothed calls; "none" is a call like any other).  A run is STRAY when it has at most q
 *   windows, is neither the first nor the last run of its record, the runs on its two sides carry the same call as each other,
 *   and each of those two has MORE than q windows.  Every stray run is decided on the unsmoothed runs (two stray runs are never
 *   adjacent: a stray run's neighbours are longer than q), so the result is a property of the call vector and nothing is iterated.
 *   A stray run's windows take their neighbours' call and their support becomes 0; keys and hit_keys stay.  Segments and mosaic
 *   are what spsp_windows_segments_host makes of the smoothed vectors: `windows` counts the absorbed windows, `support` only the
 *   windows that made the call themselves.  The windows' rows a driver hands out stay unsmoothed.
 * SELECTION.  A word: all (every segment), called (with a call), none (without), call=<b> (whose call is b), not=<b> (whose call
 *   is not b, the uncalled included), major (whose call is their record's mosaic major), minor (with a call other than none that
 *   differs from their record's major).  b is the number the segments CSV prints, b < n_bins - 1.  A record without a major
 *   selects nothing under major or minor.  A segment is written only if end - begin >= max(1, min_bases).
 * TEXT.  <prefix>_segments.fa.gz (plain <prefix>_segments.fa where gzip is off): one FASTA record per selected segment in the
 *   segments CSV's order.  Header: '>' name ':' begin + 1 '-' end ' ' call_name '\n' (1-based, inclusive; call_name as the CSV
 *   prints it).  Body: the record's kept bases [begin, end), upper case ("ACTG"[code] of the packed form), SPSP_SEGMENTS_LINE
 *   bases a line, every line ended by '\n': n bases are n + ceil(n / 80) bytes.  FASTQ input gives FASTA: the cleaned bases carry
 *   no qualities. */
#define SPSP_SEGMENTS_LINE 80u
/* What the writer cuts at (either pointer may be NULL): the bases of a line, the output bytes one workgroup owns. */
int spsp_segments_plan_host(uint32_t* line_bases, uint32_t* stretch_bytes);
/* The smoothing, in place, over the windows of n_rec records (first_win: n_rec + 1).  *n_changed (may be NULL): the windows whose
 * call changed.  SPSP_ERR_ARG naming the record for a call >= n_bins or a first_win that decreases; nothing is changed then. */
int spsp_windows_smooth_host(uint32_t* call, uint32_t* support, const uint32_t* first_win /* n_rec + 1 */, uint32_t n_rec, uint32_t n_bins, uint32_t q,
                             uint64_t* n_changed);
/* Only the refusals of a selection: `what` is a word, or the command line's <word>:<min_bases> (a decimal below 2^63).  n_bins:
 * 0 while the bins are not counted yet (then <b> is only held to be a decimal number), else b < n_bins - 1 is asked.  taxonomy:
 * the bins are nodes (for the refusal's words only). */
int spsp_segments_word_check_host(const char* what, int taxonomy, uint32_t n_bins);
/* keep[i] = 1 where segment i is selected and has at least max(1, min_bases) bases, else 0; *n_kept and *n_bases (may be NULL):
 * their number and their bases.  mosaic: the records' rows (major and minor read `major`).  SPSP_ERR_ARG for a refused word, a
 * min_bases of 2^63 or more, a segment whose record or call is out of range or whose end lies in front of its begin. */
int spsp_segments_select_host(const spsp_segment_row* segments, uint64_t n_segments, const spsp_mosaic_row* mosaic, uint32_t n_rec, uint32_t n_bins, const char* what,
                              uint64_t min_bases, uint8_t* keep /* n_segments */, uint64_t* n_kept, uint64_t* n_bases);
/* The text as plain loops over ASCII bases: the yardstick of the device writer.  bases: the cleaned bases of all records (n_bases
 * of them, written upper-cased), rec_off: n_rec + 1; keep: NULL (every segment) or a flag per segment; the names as the CSV
 * writers take them.  A segment that leaves its record is SPSP_ERR_ARG.  *text is released with spsp_free(). */
int spsp_segments_fasta_host(const uint8_t* bases, uint64_t n_bases, const uint64_t* rec_off /* n_rec + 1 */, uint32_t n_rec, const spsp_segment_row* segments,
                             uint64_t n_segments, const uint8_t* keep, const char* const* record_names, const char* const* call_names, const char* last_name,
                             uint32_t n_bins, char** text, uint64_t* len);
/* The writer on the device.  d_bases: the cleaned bases in HBM in either form the ingest writes (packed != 0: 2-bit words), 16-byte
 * aligned, with the readable bytes behind that spsp_records_windows_device asks for.  Segment i is the h_len[i] >= 1 bases from
 * global base offset h_src[i] on, behind the header h_headers[h_hdr_off[i] .. h_hdr_off[i + 1]) (the host makes the headers: only
 * it holds the names).  The host prefix-sums header and body lengths; ONE upload carries the three tables and the headers; ONE
 * launch, balanced by OUTPUT: a workgroup owns 16 KiB of the text, finds the segments that cross it by two binary searches, keeps
 * their slice of the tables in LDS, and every lane writes whole 16-byte-aligned 16-byte stores.  A store inside one body holds
 * at most one newline besides the body's last: 16 (or 15) source bases by two aligned loads and a byte shift (ASCII) or a funnel
 * shift of two dwords expanded four letters at a time (packed), the newline put in by one byte permute; byte by byte where a
 * store holds header bytes, spans segments or ends the text.  No host wait: *d_out (the context's, valid until its next call,
 * whole stretches, zero behind *n_out) is ready behind the context's stream.  SPSP_ERR_ARG before any launch for a segment that
 * leaves the bases or has no bases, and for header offsets that decrease. */
int spsp_segments_write_device(spsp_ctx* ctx, const void* d_bases, uint64_t n_bases, int packed, const uint64_t* h_src /* n_seg */, const uint64_t* h_len /* n_seg */,
                               const uint8_t* h_headers, const uint64_t* h_hdr_off /* n_seg + 1 */, uint64_t n_seg, void** d_out, uint64_t* n_out);
/* While the context's timing is on a write records events around its launch; this reads the milliseconds added up since the last
 * read and clears them (it waits for the context's stream). */
int spsp_segments_stage_ms(spsp_ctx* ctx, double* ms /* 1: write */);
/* The whole-file drivers: the arguments of the _windows entries plus smooth (q), segments_what (NULL: no text is written),
 * segments_min and gz, and the outs n_changed (windows whose call the smoothing changed), n_written (segments written) and
 * bytes_out (the text's bytes before gzip).  Behind the last batch the calls are smoothed, segments and mosaic made, the segments
 * selected and written on the second context from the bases it still holds; every text is made before any file is written.  A
 * refused word is refused before any file is read (call=<b> / not=<b>: once the bins are counted).  The two CSVs of a run with
 * a word and smooth == 0 are those of the run without.  The _windows entries are these with smooth = 0 and no word. */
int spsp_classify_files_segments(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys,
                                 uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window, const char* what,
                                 spsp_classify_record** rows, spsp_classify_hit** hits, uint64_t* n_windows, uint32_t** first_win, uint64_t* n_records,
                                 spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic, uint32_t smooth, const char* segments_what,
                                 uint64_t segments_min, int gz, uint64_t* n_changed, uint64_t* n_written, uint64_t* bytes_out);
int spsp_taxonomy_files_segments(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                                 uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window,
                                 const char* what, spsp_taxonomy_record** rows, uint64_t* n_windows, uint32_t** first_win, uint64_t* n_records,
                                 spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic, uint32_t smooth, const char* segments_what,
                                 uint64_t segments_min, int gz, uint64_t* n_changed, uint64_t* n_written, uint64_t* bytes_out);

/* ------------------------------------------------------- raw coordinates ---- */
/* Segments lifted to the positions of the file the user holds (not in the reference).  Windows and segments count only the bases
 * the ingest keeps; samtools faidx, bedtools and a genome browser count every sequence character of the record.  The map between
 * the two is a rank / select over the raw text.  Integers only.
 * SEQUENCE CHARACTERS.
 *   FASTA: a byte is a sequence character if it lies on a line that does not begin a record, and its value is 0x21 .. 0x7e.  The
 *   lines that begin a record are the extraction's rule: line 0 whatever it holds, and every line whose first byte is '>' or 0xFF.
 *   The byte range 0x21 .. 0x7e is what samtools faidx counts (isgraph).  So '\n', '\r', blanks and tabs are not counted, and N,
 *   IUPAC codes, lower case and '-' are.
 *   FASTQ: the bytes 0x21 .. 0x7e of line 4r + 1.
 *   raw_length[r] is the number of sequence characters of record r.
 *   Every kept base is a sequence character.
 * RECORDS.  A text is FASTQ when its first byte is '@', else FASTA.  FASTA: record 0 begins with the text (an empty text is one
 *   empty record, as the ingest has it), and a record begins at every later line whose first byte is '>' or 0xFF.  FASTQ: record
 *   r begins at line 4r, and a line 4r that is empty or begins with '\r' begins none: the blank lines behind the content, which
 *   the ingest sets aside, add no record.  The lines are counted through them all the same; they hold no sequence character.
 *   For every text the ingest accepts the records are the ingest's.
 * RAW POSITION.  raw(r, p) is the number of sequence characters of record r in front of its kept base number p, for
 *   0 <= p < L_r.  It is strictly increasing in p.  It equals p exactly when no other sequence character precedes the base.
 * RAW INTERVAL OF A SEGMENT.  A segment [begin, end) with end > begin has the raw interval [raw(r, begin), raw(r, end - 1) + 1).
 *   It is tight: it starts and ends on a kept base.  Ns between two segments belong to neither, since nothing was called on
 *   them.  A segment without bases (an empty record) has no raw interval.
 * BED.  <prefix>_segments.bed.gz (plain <prefix>_segments.bed where gzip is off): one line per segment that has bases, in the
 *   segments CSV's order, tab-separated: name, raw_begin, raw_end, call_name, 0, ., segment, begin, end, windows, support -- BED6
 *   and five columns; raw_begin is 0-based and raw_end exclusive, as BED has it; call_name is what the CSV prints, a tab inside it
 *   written as a blank. */
/* What the kernels cut at (either pointer may be NULL): the bytes of the text per workgroup and per lane (the ingest's). */
int spsp_lift_plan_host(uint32_t* tile_bytes, uint32_t* chunk_bytes);
/* The rule as plain loops: the yardstick of the device pass.  h_base[q]: GLOBAL kept-base indices (rec_off[r] + p, the numbering
 * spsp_segments_write_device takes in h_src), non-decreasing, equal values allowed.  raw[q]: record-relative; rec[q] (may be
 * NULL): the record that holds the base; raw_length (may be NULL): on entry *n_rec is the records it has room for, and a text
 * that holds another number is SPSP_ERR_ARG; *n_rec: the records of the text.  SPSP_ERR_ARG for indices that decrease and for an
 * index that is not below the text's kept bases; the outputs then hold nothing to use. */
int spsp_records_lift_host(const uint8_t* text, uint64_t n, const uint64_t* h_base /* n_q */, uint64_t n_q, uint64_t* raw /* n_q, caller's */,
                           uint32_t* rec /* n_q, may be NULL */, uint64_t* raw_length /* n_rec, may be NULL */, uint32_t* n_rec);
/* The BED text.  raw_begin, raw_end: one per segment (read only for segments that have bases).  SPSP_ERR_ARG for a segment whose
 * record or call is out of range, and for a raw interval shorter than the segment's bases.  *text is released with spsp_free(). */
int spsp_segments_bed_host(const spsp_segment_row* segments, uint64_t n_segments, const uint64_t* raw_begin, const uint64_t* raw_end, const char* const* record_names,
                           uint32_t n_rec, const char* const* call_names, const char* last_name, uint32_t n_bins, char** text, uint64_t* len);
/* The pass on the device.  d_text: the raw text in HBM, 16-byte aligned as the extraction asks; n_bases: the kept bases the ingest
 * counted for it; the arrays as above, in host memory.  Launches: per 4 KiB tile (a lane per 16-byte chunk) the line-state
 * transform and, per state the tile may be entered in, its kept bases, sequence characters and record starts (FASTQ: the newline
 * count takes the transform's place, so the line phase mod 4 is additive); one workgroup scan -> every tile's entry state and
 * its prefixes K, S, R; the answer, a workgroup per tile: two binary searches over the uploaded indices name its queries,
 * K[t] <= g < K[t + 1] (a tile without a kept base has none, so a query goes to the tile that holds its base), and a tile without
 * queries leaves at once; the others rebuild the chunks' exclusive prefixes in LDS, a lane per query searches the 256 prefixes,
 * finds the bit of the chunk's keep mask by popcounts and counts the sequence-mask bits below it; the same launch over R, with
 * the queries' records as its queries, finds the sequence prefix at each of those records' starts (a lane per start of the
 * tile, which answers the first query of its record; where raw_length is asked, once more for every record); a lane per query
 * finds its record's first query and subtracts.  ONE upload, ONE host wait.  Work is balanced by input bytes.
 * Loads are guarded by n_text; plain vector stores, no atomics.
 * Refused with SPSP_ERR_ARG before any launch: a text that is not 16-byte aligned, indices that decrease, n_q > 0 with
 * n_bases == 0, raw_length with room for no record.  Refused with SPSP_ERR_ARG behind the wait: an index >= n_bases, an n_bases
 * that is not what the pass itself counts for the text, a record count that is not raw_length's room.  n_q == 0 launches nothing
 * (and *n_rec is 0), unless raw_length is asked for. */
int spsp_records_lift_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, uint64_t n_bases, const uint64_t* h_base /* n_q */, uint64_t n_q,
                             uint64_t* raw /* n_q, caller's */, uint32_t* rec /* n_q, may be NULL */, uint64_t* raw_length /* n_rec, may be NULL */, uint32_t* n_rec);
/* While the context's timing is on a lift records events between its launches; this reads the milliseconds added up since the
 * last read and clears them. */
int spsp_lift_stage_ms(spsp_ctx* ctx, double* ms /* 3: count, scan, answer */);
/* The whole-file drivers: the arguments of the _segments entries plus raw, the outs raw_begin and raw_end (one per segment, 0 for
 * a segment without bases; spsp_free; may be NULL; handed out only where raw is asked) and bed_bytes (the BED text's bytes before
 * gzip; may be NULL).  With raw != 0, behind the last batch and the smoothing, the two ends of every segment that has bases go
 * through ONE spsp_records_lift_device call on the second context, over the text it still holds, and <out_prefix>_segments.bed
 * (".gz" appended when gz) is written beside the CSVs; every text is made before any file is written.  Both CSVs and the
 * segments' FASTA of a run with raw are those of the run without.  The _segments entries are these with raw = 0. */
int spsp_classify_files_raw(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys, uint32_t num,
                            uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window, const char* what,
                            spsp_classify_record** rows, spsp_classify_hit** hits, uint64_t* n_windows, uint32_t** first_win, uint64_t* n_records,
                            spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic, uint32_t smooth, const char* segments_what,
                            uint64_t segments_min, int gz, uint64_t* n_changed, uint64_t* n_written, uint64_t* bytes_out, int raw, uint64_t** raw_begin,
                            uint64_t** raw_end, uint64_t* bed_bytes);
int spsp_taxonomy_files_raw(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path, uint32_t min_keys,
                            uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window, const char* what,
                            spsp_taxonomy_record** rows, uint64_t* n_windows, uint32_t** first_win, uint64_t* n_records, spsp_segment_row** segments,
                            uint64_t* n_segments, spsp_mosaic_row** mosaic, uint32_t smooth, const char* segments_what, uint64_t segments_min, int gz,
                            uint64_t* n_changed, uint64_t* n_written, uint64_t* bytes_out, int raw, uint64_t** raw_begin, uint64_t** raw_end, uint64_t* bed_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SPSP_H */
