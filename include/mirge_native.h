/*
 * mirge_native.h -- C ABI of libmirge_native.so: the MI355X (gfx950) implementation of the
 * miRge3.0 hot path (collapse -> annotation cascade -> count join).
 *
 * The reference (mhalushka/miRge3.0) has no FFI for this path: it is three Python call sites
 * and one process boundary.  Each entry point below names what it replaces;
 * INTEGRATION.md shows the ctypes stub a miRge3.0 maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative code on failure; mirge_last_error()
 *     returns the message of the calling thread's last failure (the reference either raises
 *     CalledProcessError from subprocess.run(check=True), manifoldAlign.py:19, or prints and
 *     exits; the Python wrapper turns a non-zero code into RuntimeError);
 *   - plain pointers and sizes only; "host" pointers are ordinary process memory (numpy
 *     buffers), all device memory is owned by the opaque handles;
 *   - sequences cross the boundary as one ASCII byte array plus int64 offsets[n+1];
 *   - handles are created/destroyed by the library, the caller allocates every output array;
 *   - one mirge_ctx = one GPU + one HIP stream; calls on one ctx are serialised by the caller,
 *     different ctx (different GPUs) may be driven from different threads/processes.
 */
#ifndef MIRGE_NATIVE_H
#define MIRGE_NATIVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mirge_ctx mirge_ctx;       /* device + stream + workspace pool              */
typedef struct mirge_lib mirge_lib;       /* one reference library, packed + indexed in HBM */
typedef struct mirge_reads mirge_reads;   /* device-resident packed read set (+ counts)     */
typedef struct mirge_result mirge_result; /* device-resident per-read annotation            */

/* One cascade pass = one of the ten bowtie argument strings of manifoldAlign.py:85, restated
 * (SURVEY.md 8 table a8-P).  Same fields as oracle_policy minus the annotFlag test, which the
 * cascade applies itself (manifoldAlign.py:120,129). */
typedef struct mirge_policy {
    int32_t mode;     /* 0: -n N (seeded), 1: -v V (end to end)                          */
    int32_t mm;       /* N or V                                                          */
    int32_t seedlen;  /* -l, bowtie default 28                                           */
    int32_t maxtotal; /* -n: 2 (FASTA Q40 -> Maq-rounded 30, -e 70); -v: V               */
    int32_t trim5;    /* -5                                                              */
    int32_t trim3;    /* -3                                                              */
    int32_t ttail;    /* 1: only reads matching T{3,}$, aligned without that run (:118-126) */
    int32_t len_lt;   /* >0: only reads shorter than this (pass 0: 26, :93)              */
    int32_t len_gt;   /* >0: only reads longer than this (pass 1: 25, :104)              */
    int32_t reserved;
} mirge_policy;

#define MIRGE_MAX_PASSES 16
#define MIRGE_NO_PASS (-1)

const char* mirge_last_error(void);

/* replaces: miRgeEssential.check_dependencies probing `bowtie --version` (miRgeEssential.py:6-34) */
int mirge_device_count(void);
/* hip_stream: a hipStream_t to run on (e.g. torch's current stream) or NULL for a private one */
int mirge_ctx_create(int device, void* hip_stream, mirge_ctx** out);
/* Ownership: libraries, read sets and results hold device blocks of the context they were made in -- destroy them BEFORE the
   context (the ctypes binding does that by itself: closing a Context closes what still lives in it).  A cascade may be handed
   a library of ANOTHER context of the same device (its probe tables are shared under the library's lock); the whole-read tables
   of the exact passes are built, named and dropped only through the context the library was made in -- a borrower's exact
   passes take the probe path, with the same results. */
void mirge_ctx_destroy(mirge_ctx* ctx);
int mirge_ctx_sync(mirge_ctx* ctx);
/* out[0] = bytes the pool has from the driver, out[1] = blocks handed out and not back, out[2] = blocks in the free list.
 * Host bookkeeping only: queues nothing, waits for nothing.  Deferred blocks count as handed out until a join returns them. */
int mirge_ctx_pool_stats(mirge_ctx* ctx, int64_t out[3]);

/* ---- libraries: replaces `bowtie <index>` opening an .ebwt index (manifoldAlign.py:97-99)
 * and `bowtie-build`.  seq_ascii/offsets: the reference sequences in library order.          */
int mirge_lib_create(mirge_ctx* ctx, const char* seq_ascii, const int64_t* offsets, int64_t n_refs,
                     mirge_lib** out);
/* The same from the packed image mirge_lib_create derives (2-bit text, invalid-base bitmap, reference starts): what a
 * library cache next to the index holds, so that a process neither parses the FASTA / decodes the .ebwt nor packs it
 * again.  mirge_lib_packed_sizes / _copy hand the image of a library out (sizes[4] = words of T, words of inv, total
 * bases incl. separators, valid positions).  Probe tables are built on the device either way. */
int mirge_lib_create_packed(mirge_ctx* ctx, const uint64_t* T, int64_t n_T, const uint64_t* inv, int64_t n_inv,
                            const uint32_t* ref_start, int64_t n_refs, uint64_t total, int32_t kmax,
                            uint64_t valid_positions, mirge_lib** out);
int mirge_lib_packed_sizes(const mirge_lib* lib, int64_t* sizes, int32_t* kmax);
int mirge_lib_packed_copy(const mirge_lib* lib, uint64_t* T, uint64_t* inv, uint32_t* ref_start);
void mirge_lib_destroy(mirge_lib* lib);
int64_t mirge_lib_n_refs(const mirge_lib* lib);
int64_t mirge_lib_device_bytes(const mirge_lib* lib);
/* build the k-mer table for probe length k now (otherwise built on first need) */
int mirge_lib_prepare(mirge_lib* lib, int32_t k);

/* ---- input: a whole .gz file's bytes -> its text on `threads` host threads (0: all).  What xopen's pigz / igzip threads are to the
 * reference's reader (digest.py:136-140): one zlib stream inflates at ~0.4 GB/s of text, twenty times slower than everything
 * behind it here.  An ordinary member is cut at deflate block starts found by search and decoded in parallel (csrc/native_gz.hpp);
 * a BGZF file member by member.  out[cap]; 0 = done and verified against the file's own CRC-32 and length; negative = not
 * taken by this route (several ordinary members, too small, not text, damaged, cap too small): inflate it serially. */
int mirge_gz_inflate(const uint8_t* gz, int64_t n_gz, uint8_t* out, int64_t cap, int64_t* n_out, int32_t threads);
/* the same; while it runs `*progress` (may be NULL) is advanced to the number of leading bytes of `out` that are final, so that a
 * second thread can upload and parse whole records of that prefix beside the inflation (the reference's reader hands chunks to its
 * workers while xopen's threads inflate, digest.py:136-140).  The CRC-32 is verified at the end: on a negative return whatever was
 * read ahead must be dropped. */
int mirge_gz_inflate_progress(const uint8_t* gz, int64_t n_gz, uint8_t* out, int64_t cap, int64_t* n_out, int32_t threads, int64_t* progress);

/* ---- reads: replaces writing bwtInput.fasta (manifoldAlign.py:92-95) / dnaio parsing ---- */
int mirge_reads_pack(mirge_ctx* ctx, const char* ascii, const int64_t* offsets, int64_t n,
                     mirge_reads** out);
/* The same from the FILE's text, parsed on the device: replaces dnaio's record parsing and the length filter of the
 * per-chunk worker (digest.py:320-375, --minimum-length :348,368).  format: 1 FASTQ (4-line records), 2 FASTA (one
 * sequence line per record), 3 one sequence per line, 0 = by the first byte.  *n_records = records seen before the
 * filter (`count`, digest.py:326).  Reads come out in file order.  A read may be up to 65 535 nt (the reference has no upper
 * bound -- parse.py:102 `-M` is never read, digest.py:348,368 test the minimum only --; reads beyond 255 nt take kernels written
 * for any length, csrc/kernels_long.hpp); a longer one is refused (-6). */
int mirge_reads_parse(mirge_ctx* ctx, const char* text, int64_t nbytes, int32_t format, int32_t min_len,
                      mirge_reads** out, int64_t* n_records);
/* 1 when some read of the set held an IUPAC ambiguity code other than N: such a base is packed -- and later printed --
 * as N (bowtie aligns it as N too; the reference's dictionary would have kept the letter). */
int32_t mirge_reads_iupac_seen(const mirge_reads* reads);
/* The same with the read modifiers the reference runs through cutadapt before it counts a read (digest.py:59-101; SURVEY.md
 * 8f row N4), applied on the device between record finding and the length filter: NextSeq quality trimming, quality
 * trimming, adapter removal (one or two adapters, 3' or 5', regular or anchored, or one linked adapter), N trimming,
 * unconditional cuts -- in that order, each present when its field says so.
 * count_per_modifier = 1 reproduces the reference's worker at HEAD, which tests the length and counts the read after
 * EVERY modifier (digest.py:354-373); 0 counts the fully trimmed read once.  *n_records stays the number of records of
 * the text.  trim == NULL: mirge_reads_parse.  Restated from cutadapt's published algorithms: parity unpinned. */
typedef struct mirge_trim {
    int32_t nextseq_cutoff;   /* --nextseq-trim, -1 = off                                   */
    int32_t quality_front;    /* -q 5'CUTOFF (0 when only one value is given)                */
    int32_t quality_back;     /* -q 3'CUTOFF (the reference's default: 10), -1 = off         */
    int32_t phred_base;       /* 33 (or 64)                                                  */
    const char* adapter;      /* -a: 3' adapter, A/C/G/T/N (or -g, see adapter_front), or NULL */
    int32_t adapter_len;
    int32_t min_overlap;      /* --overlap (3)                                               */
    double error_rate;        /* --error-rate (0.12), of the aligned adapter length          */
    int32_t trim_n;           /* --trim-n                                                    */
    int32_t n_cut;            /* -u, up to two values: > 0 from the 5' end, < 0 from the 3'  */
    int32_t cut[2];
    int32_t count_per_modifier;
    int32_t adapter_front;    /* 1: `adapter` is a 5' adapter (-g): the read keeps what follows it; no N */
    const char* adapter2;     /* a second adapter or NULL: per read the better match of the two is removed (cutadapt's   */
    int32_t adapter2_len;     /* AdapterCutter with times = 1: most matches, then fewest errors, then the first given)  */
    int32_t adapter2_front;
    int32_t times;            /* -n COUNT: remove adapters up to COUNT times (0 / 1: once)                               */
    int32_t no_indels;        /* --no-indels: substitutions only in the adapter alignment                                 */
    int32_t match_read_wildcards;  /* --match-read-wildcards: an N in the read matches every adapter base                  */
    int32_t no_adapter_wildcards;  /* -N: an N in the adapter is not a wildcard                                            */
    int32_t action_none;      /* --action none: adapters are searched, the read is left as it is                          */
    /* anchored and linked adapters, as cutadapt's parser makes them of the specification strings the reference hands through
     * unchanged (digest.py:66-84; docs/source/quick_start.md:213-220 shows `-g "TTAGGC...TGGAATTCTCGGGTGCCAAGGAACTCCAGT"`):  */
    int32_t adapter_anchored; /* `-g ^ADAPTER`: the whole adapter at the read's first base / `-a ADAPTER$`: up to its last base */
    int32_t adapter2_anchored;
    int32_t linked;           /* 1: `adapter` (adapter_front = 1) and `adapter2` (3') are the two parts of ONE linked adapter
                               * ADAPTER1...ADAPTER2: the 5' part is searched first, the 3' part in what follows it             */
    int32_t linked_required;  /* bit 0: no match without the 5' part, bit 1: without the 3' part (`-a A...B`: 1, `-g A...B`: 3)  */
} mirge_trim;
int mirge_reads_parse_trim(mirge_ctx* ctx, const char* text, int64_t nbytes, int32_t format, int32_t min_len,
                           const mirge_trim* trim, mirge_reads** out, int64_t* n_records);
/* The same with the reference's UMI handling: replaces the UMI branches of the per-chunk worker
 * (digest.py:334-365), `UMIParser` (:305-315) and the UMI stage of baking (:164-205) for one file.
 *   front, back  -umi f,b: read[f : len - b] is the insert (Python's s[f:-b]; s[f:] when b == 0), the rest the UMI
 *   qiagen       --qiagenumi (:334-352): the dictionary key is the trimmed read + the `back` bases that follow the 3'
 *                adapter in the untrimmed line (`currentSeq.split(trimmed)[1][:len(adapter)+b][-b:]`, first occurrence,
 *                "" when the trimmed read is empty); counted once, after the last modifier; needs trim->adapter (3')
 *   dedup        -udd (:183-205): a count is a number of distinct UMI-tagged reads; 2: -udd with directional clustering (below)
 * The worker's length test applies to the insert (`len(pureSeq) >= min_len`, :360), with qiagen to the trimmed read (:349),
 * and baking's to the insert again (:173,192).
 * *out: RAW inserts in file order -- without dedup one per counted read; with dedup one per DISTINCT tagged read whose
 * insert passes, in the order the tagged reads first appeared, so that mirge_collapse of *out gives molecule counts and
 * first indices that are ranks in the reference's dictionary order.  mirge_reads_count(*out) = 'Trimmed Reads (all)'.
 * *tagged_out (dedup only; may be NULL): the distinct tagged reads with their counts (a collapse result): the rows of
 * <sample>_umiCounts.csv (:183-197) are those whose insert passes the length test.  umi == NULL: mirge_reads_parse_trim. */
typedef struct mirge_umi {
    int32_t front;
    int32_t back;
    int32_t qiagen;
    int32_t dedup;
} mirge_umi;
int mirge_reads_parse_umi(mirge_ctx* ctx, const char* text, int64_t nbytes, int32_t format, int32_t min_len,
                          const mirge_trim* trim, const mirge_umi* umi, mirge_reads** out, int64_t* n_records,
                          mirge_reads** tagged_out);
/* Error-tolerant UMI deduplication (--umi-cluster directional): the "directional" network method of UMI-tools (Smith, Heger &
 * Sudbery 2017) on the distinct tagged reads of one sample.  `tagged`: any collapse result with ONE count column (*tagged_out above,
 * or mirge_collapse[_weighted] of packed reads); the UMI is a read's first `front` and last `back` letters, 1 <= front + back <= 32.
 * A read is eligible iff it holds no N, has at most 256 nt and at least front + back; two eligible reads of one length that differ in
 * exactly one letter, inside the UMI, are neighbours; edge a -> v iff count(a) >= 2 count(v) - 1 (64-bit).  founder_out (host,
 * [mirge_reads_count(tagged)], handle order) = 1 for every ineligible read, every read of count >= 2 without an edge into it, and the
 * earliest member (smallest first index) of every connected component of count-1 reads none of whose members has a neighbour of count
 * >= 2: as many founders among an insert's eligible reads as UMI-tools' searches.  *n_founders = the ones in founder_out.
 * mirge_umi.dedup == 2 makes mirge_reads_parse_umi call the same routine: *out then holds the inserts of the founders only, in the order
 * the founders first appeared; *tagged_out is what dedup == 1 gives.
 * mirge_umi_cluster_stats: out[0..4] = tagged reads, eligible reads, count-1 reads with a count-1 neighbour, rounds of the label
 * propagation and slots of the lookup table of this thread's last clustering. */
int mirge_umi_cluster(mirge_ctx* ctx, const mirge_reads* tagged, int32_t front, int32_t back, uint8_t* founder_out, int64_t* n_founders);
int mirge_umi_cluster_stats(int64_t* out);
/* --kmer-correct: k-mer spectrum error correction of one sample's distinct reads.  uniq: a collapse result with one count column.
 * Rounds run for k = k_start .. k_end (8 <= k_start <= k_end <= 31), each on the dictionary the round before left.  In a round a read is
 * eligible iff it holds no N and has k .. 256 nt; S(x) = the sum of the counts of the eligible reads over every window that spells the
 * k-mer x (forward strand, 64-bit); a window is weak iff S <= threshold (>= 1).  A read with a weak window is suspect; with lo = its last
 * weak start and hi = its first weak start + k - 1 it is uncorrectable if lo > hi, else every (p, b), lo <= p <= hi, p < len, b != r[p],
 * is a candidate: valid iff every window of the changed read that covers p is solid, scored by the smallest S among them.  The read is
 * corrected iff exactly one valid candidate has the largest score (none: unsupported; several: ambiguous).  The corrected reads are
 * regrouped: counts add, the first index is the smallest of the contributors'.  *out: the dictionary after the last round (a collapse
 * result of its own, to be destroyed by the caller; its first indices are those of `uniq`).  final_of (host, [mirge_reads_count(uniq)],
 * or NULL): the handle index in *out of every read of uniq; rounds_mask (the same shape, or NULL): bit (k - k_start) set iff the read,
 * or the read it had become by then, was corrected in the round of k.  MIRGE_TEST_EC_HASH_BITS=N keeps N bits of the hashes (tests).
 * mirge_kmer_correct_stats: out[8 r + 0..7] for round r of this thread's last call = eligible, suspect, corrected, uncorrectable,
 * unsupported and ambiguous reads, distinct reads after the round, slots of the round's table; returns the number of rounds (<= 24). */
int mirge_kmer_correct(mirge_ctx* ctx, const mirge_reads* uniq, int32_t k_start, int32_t k_end, int32_t threshold, mirge_reads** out,
                       uint32_t* final_of, uint32_t* rounds_mask);
int mirge_kmer_correct_stats(int64_t* out);
/* --kmer-ratio R: mirge_kmer_correct with a relative threshold.  ratio == 0 is exactly mirge_kmer_correct; ratio == 1 and ratio < 0 are
 * refused.  With ratio >= 2 a window has a second way to be weak, decided on the round's spectrum before anything else:
 *   2a. a k-mer x with S(x) > threshold is DOMINATED iff a k-mer y that differs from x in exactly one letter has S(y) >= ratio * S(x)
 *       (exact integers: the product is never formed where it would not fit 64 bits; floor(S(y) / ratio) >= S(x) is the same predicate);
 *   2b. x is weak iff S(x) <= threshold or x is dominated; else solid.
 * Domination is decided from the sums alone: y may itself be dominated; a k-mer no eligible read holds has sum 0 and dominates nothing.
 * All else is as above; a candidate's score is still the smallest S among windows that are all solid.
 * mirge_kmer_correct_ratio_stats: out[2 r + 0..1] for round r of this thread's last call = distinct k-mers with S > threshold, the
 * dominated among them (zeros when that call had no ratio); returns the number of rounds (<= 24). */
int mirge_kmer_correct_ratio(mirge_ctx* ctx, const mirge_reads* uniq, int32_t k_start, int32_t k_end, int32_t threshold, int32_t ratio,
                             mirge_reads** out, uint32_t* final_of, uint32_t* rounds_mask);
int mirge_kmer_correct_ratio_stats(int64_t* out);
/* -a auto: a sample's 3' adapter from the distinct reads of its head (README, "`-a auto`: the 3' adapter, inferred from the reads").  uniq: a
 * collapse result with ONE count column (more: an error), made of UNTRIMMED reads.  A read without N of 12 .. 256 letters is eligible;
 * T = the sum of their counts; for a 12-mer x, C(x) = the sum of the counts over every window start p <= 63 that spells x and M(x) the
 * mask of those p.  The seed is the 12-mer with the largest C among those with three distinct letters, popcount(M) >= 6 and
 * C >= max(32, ceil(T / 20)) (equal C: the smallest string); up to 64 steps to the left while a letter in front keeps popcount(M) >= 6
 * and 10 C >= 9 C(current); then to the right, up to 32 letters, while a letter behind has 2 C >= C(start).  No candidate, or an empty
 * dictionary: seq is empty, len 0 (T and candidates are still reported).  Codes have the first letter most significant (A C G T =
 * 0 1 2 3).  probe (n_probe codes, may be NULL with 0): probe_sum[q] / probe_mask[q] = C and M of code probe[q] (a code >= 4^12: zeros). */
typedef struct mirge_adapter {
    char seq[40];          /* NUL-terminated; empty: no adapter */
    int32_t len, left_steps, spread, pad; /* letters; steps of the left walk; popcount(M(start)) */
    uint64_t support;      /* C(start) */
    uint64_t eligible;     /* T */
    uint64_t seed_sum;     /* C(seed) */
    uint64_t candidates;   /* seed candidates */
    uint32_t seed, start;  /* codes, first letter most significant */
} mirge_adapter;
int mirge_adapter_infer(mirge_ctx* ctx, const mirge_reads* uniq, mirge_adapter* out, const uint32_t* probe, int64_t n_probe, uint64_t* probe_sum,
                        uint64_t* probe_mask);
/* Several raw read sets as one, in the order given (the samples of a run, one file each, before the joint collapse
 * that replaces the per-file dicts and their outer join, digest.py:133-163,243).  The parts stay valid. */
int mirge_reads_concat(mirge_ctx* ctx, const mirge_reads* const* parts, int32_t n_parts, mirge_reads** out);
void mirge_reads_destroy(mirge_reads* reads);
int64_t mirge_reads_count(const mirge_reads* reads);
int64_t mirge_reads_total_bases(const mirge_reads* reads);
int32_t mirge_reads_n_samples(const mirge_reads* reads);
/* reads per storage group (width class x {no ambiguous call, has an N}): out[0 .. min(cap, groups)), returns the
 * number of groups.  Diagnostics and bench.py's units: "collapsed reads of the bulk group" is the largest entry. */
int32_t mirge_reads_group_counts(const mirge_reads* reads, int64_t* out, int32_t cap);
/* sequences back as ASCII: ascii_out[total_bases], offsets_out[n+1], in handle order */
int mirge_reads_unpack(mirge_ctx* ctx, const mirge_reads* reads, char* ascii_out, int64_t* offsets_out);

/* ---- collapse: replaces the dict merge of digest.py:141-163 and the sample matrix of
 * digest.py:237-245.  sample_ids[n] (host, may be NULL when n_samples == 1) gives the sample
 * of every raw read.  The result holds the U distinct sequences (grouped by width class; their order
 * inside a group is unspecified -- sort by first_index for the reference's dict order) and a
 * U x n_samples count matrix.                                                              */
int mirge_collapse(mirge_ctx* ctx, const mirge_reads* raw, const int32_t* sample_ids,
                   int32_t n_samples, mirge_reads** uniq, int64_t* n_uniq);
/* The same where raw read i stands for weights[i] (host, >= 1) copies: merges already collapsed dictionaries -- the
 * per-sample results a sharded run gathers on rank 0 -- into the sample matrix (the outer join of digest.py:243)
 * without expanding them.  first indices refer to the raw set as given. */
int mirge_collapse_weighted(mirge_ctx* ctx, const mirge_reads* raw, const int32_t* sample_ids, int32_t n_samples,
                            const uint32_t* weights, mirge_reads** uniq, int64_t* n_uniq);
/* The sample matrix of several samples from their per-sample dictionaries, entirely on the device (round 6; what the CLI's route for
 * several files calls): parts[s] = the collapse result of sample s alone (one count column); -> the unique reads of the union with an
 * n_parts-column count matrix, as mirge_collapse with sample ids over the samples' raw reads would give -- the outer join of
 * mirge/libs/digest.py:243 -- without putting the raw reads of all samples through one table.  The parts stay valid. */
int mirge_collapse_merge(mirge_ctx* ctx, const mirge_reads* const* parts, int32_t n_parts, mirge_reads** uniq, int64_t* n_uniq);
/* counts_out[U * n_samples] (row-major), first_index_out[U] (index of the first raw read, may be NULL) */
int mirge_collapse_fetch(mirge_ctx* ctx, const mirge_reads* uniq, uint32_t* counts_out,
                         int64_t* first_index_out);
/* order_out[k] (k < U) = index of the unique read that appeared k-th in the raw reads: the row order of the reference's
 * per-sample dictionary (insertion order, digest.py:158-163), from one device sort of the first indices. */
int mirge_collapse_order(mirge_ctx* ctx, const mirge_reads* uniq, int64_t* order_out);
/* order_out[k] (k < U) = index of the unique read in row k of the SORTED union of the sequences (Python string order): the
 * row order of the sample matrix of several samples (pandas `join(how='outer')` sorts its index, digest.py:243), from a
 * radix sort on the device instead of a host-side sort of U strings. */
int mirge_collapse_order_sorted(mirge_ctx* ctx, const mirge_reads* uniq, int64_t* order_out);
/* nonzero_out[n_samples] = unique reads with a count in each sample ('Trimmed Reads (unique)', digest.py:214) */
int mirge_collapse_nonzero(mirge_ctx* ctx, const mirge_reads* uniq, int64_t* nonzero_out);
/* attach a caller-made count matrix (U x n_samples, host) to a packed read set, e.g. after -rr */
int mirge_reads_set_counts(mirge_ctx* ctx, mirge_reads* reads, const uint32_t* counts, int32_t n_samples);

/* ---- cascade: replaces bwtAlign + alignPlusParse (manifoldAlign.py:12-146): the n_pass
 * bowtie runs, their FASTA/SAM round trips and the DataFrame updates.  libs[p] == NULL skips
 * pass p.  Every pass sees the rows no earlier pass annotated (the reference tests annotFlag only from
 * pass 2 on, :120,129, but its passes 0 and 1 are disjoint by length, :93,104, so this is the same).  Result per read: pass index (or MIRGE_NO_PASS), reference index in libs[pass],
 * 0-based offset in that reference, mismatches.
 * The call returns with the small read groups' streams not yet joined into the ctx stream: the library's next entry point on
 * this ctx makes the join (mirge_count_join puts the bulk read group's part of its work in front of it).  Work the CALLER
 * enqueues on that stream is ordered behind a cascade only after such a call (mirge_ctx_sync, for one).  */
int mirge_cascade_run(mirge_ctx* ctx, const mirge_reads* reads, const mirge_lib* const* libs,
                      const mirge_policy* policies, int32_t n_pass, mirge_result** out);
/* optional: build NOW what a cascade over `reads` (raw or collapsed: only the read lengths present matter) builds on first
 * use -- merged libraries, probe tables, plan tables -- and wait for it.  The reference pays this as bowtie-build, once per
 * library release; here it is device work of a process's first sample (timed separately by bench.py's cli_path). */
int mirge_cascade_prepare(mirge_ctx* ctx, const mirge_reads* reads, const mirge_lib* const* libs, const mirge_policy* policies,
                          int32_t n_pass);
/* How the ctx's current cascade configuration (the last mirge_cascade_prepare / _run / mirge_collapse_cascade) walks the bulk
 * group of one-word reads: walks[0] = walks over its survivor list, walks[1] = passes answered by one whole-read lookup
 * ("-v 0", or "-n 0" inside the seed, over a small library: manifoldAlign.py:85 passes 0 and 3) that ride in another pass's
 * walk, walks[2] = passes in all.  Nothing in the reference corresponds to it: diagnostics for tests and bench.py. */
int mirge_cascade_walks(mirge_ctx* ctx, int32_t* walks);
/* Test / measurement aid: the constant-rate clock ticks every workgroup of the last PROFILED bulk-cascade launch took (its
 * segment of the reads through all passes), ticks_out[0 .. min(cap, *grid_out)), and the clock's rate in kHz: the longest
 * workgroup's share of the launch says whether one read's candidate list is what the launch waited for. */
int mirge_cascade_wg_times(mirge_ctx* ctx, uint32_t* ticks_out, int32_t cap, int32_t* grid_out, int32_t* khz_out);
/* mirge_collapse followed by mirge_cascade_run for ONE sample, as one call: the bulk read group's passes are queued on
 * the GPU behind the collapse kernels before the host has read the unique counts back (the kernels take the count
 * from device memory), so the GPU does not idle across the collapse's host synchronisation.  Same results; falls
 * back to the two calls when the bulk group is not on the partitioned key path.  Replaces the baking -> bwtAlign
 * hand-over of mirge/__main__.py:140-157 for a single sample. */
int mirge_collapse_cascade(mirge_ctx* ctx, const mirge_reads* raw, const mirge_lib* const* libs, const mirge_policy* policies,
                           int32_t n_pass, mirge_reads** uniq, int64_t* n_uniq, mirge_result** out);
int mirge_result_fetch(mirge_ctx* ctx, const mirge_result* res, int8_t* pass_out, int32_t* ref_out,
                       int32_t* off_out, int8_t* mm_out);
void mirge_result_destroy(mirge_result* res);

/* ---- count join: replaces the pandas sums of summary.py:686-698 (per-class), :749-752
 * (exact / isomiR group-by) and :769-771.  class_sums[n_pass * S]; exact/iso[n_mirna * S]
 * accumulate the counts of reads annotated in exact_pass / iso_pass per reference.          */
int mirge_count_join(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res,
                     int32_t exact_pass, int32_t iso_pass, int64_t n_mirna,
                     int64_t* class_sums, int64_t* exact, int64_t* iso);

/* same sums from host arrays (the reference's summarize() is handed a DataFrame, summary.py:677):
 * pass[n] (MIRGE_NO_PASS = unannotated), ref[n], counts[n * S] row-major                   */
int mirge_count_join_host(mirge_ctx* ctx, const int8_t* pass, const int32_t* ref, const uint32_t* counts,
                          int64_t n, int32_t n_samples, int32_t n_pass, int32_t exact_pass, int32_t iso_pass,
                          int64_t n_mirna, int64_t* class_sums, int64_t* exact, int64_t* iso);

/* ---- the per-read tables: replaces pdMapped.to_csv / pdUnmapped.to_csv (mirge/__main__.py:164-173) and the U-row
 * DataFrame of Python strings they print.  Host arrays in (what mirge_reads_unpack / mirge_result_fetch /
 * mirge_collapse_fetch returned), the reference's bytes out, formatted on the host's cores.  rows[k] = read printed in
 * row k; a read with pass >= 0 goes to mapped_path, the others to unmapped_path (either may be NULL).  Columns:
 * Sequence, annotFlag, n_name_cols name columns (pass p writes its reference name into column col_of_pass[p]),
 * S counts.  name_data[p] / name_off[p] / name_n[p]: the reference names of pass p's library.  No GPU involved. */
int mirge_annotation_csv(const char* mapped_path, const char* unmapped_path, const char* header,
                         const char* seq_ascii, const int64_t* seq_off, const int8_t* pass, const int32_t* ref,
                         const uint32_t* counts, int32_t n_samples, const int64_t* rows, int64_t n_rows,
                         int32_t n_pass, const int32_t* col_of_pass, int32_t n_name_cols,
                         const char* const* name_data, const int64_t* const* name_off, const int64_t* name_n);

/* The same two files straight from the device-resident run (what the CLI's route calls): the rows are formatted by kernels
 * from the packed unique reads, their count matrix and the cascade's annotation, only the files' text crosses PCIe.
 * rows / header / columns / names as above.  Returns -4 when a reference name would need CSV quoting: format on the host. */
int mirge_annotation_csv_device(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const char* mapped_path,
                                const char* unmapped_path, const char* header, const int64_t* rows, int64_t n_rows,
                                int32_t n_pass, const int32_t* col_of_pass, int32_t n_name_cols,
                                const char* const* name_data, const int64_t* const* name_off, const int64_t* name_n);

/* ---- the sharded run's parallel tail (round 6).  The reference's ONE mapped.csv / unmapped.csv hold the sorted union of all
 * samples' sequences with one count column per sample (the outer join of mirge/libs/digest.py:243, written at
 * mirge/__main__.py:164-173).  With one sample per GPU the union's key space is cut into one range per rank by the first 21
 * bases of that order; every rank merges, annotates, orders and formats ITS stretch of the two files.
 *   mirge_reads_range_sample   k evenly spaced quantiles of a dictionary's first-word sort keys (3 bits per base: end 0, A 1, C 2,
 *                              G 3, N 4, T 5; 21 bases, most significant first -- Python's string order).  The ranks pool them.
 *   mirge_reads_range_split    the dictionary as host arrays ordered by (owner range, handle index): range q =
 *                              [splitters[q-1], splitters[q]) of that key; bounds_out[q] .. bounds_out[q+1] are its rows.
 *                              ascii_out / off_out as mirge_reads_unpack, counts_out [n][n_samples].  n_parts <= 256.
 *   mirge_annotation_csv_device_sizes   bytes_out[0] / [1] = bytes the listed rows take in mapped.csv / unmapped.csv.
 *   mirge_annotation_csv_device_at      the rows' text at the given offsets of the two EXISTING files (no header, no
 *                                       truncation): the caller created them at their final size from every rank's sizes. */
int mirge_reads_range_sample(mirge_ctx* ctx, const mirge_reads* uniq, int32_t k, uint64_t* keys_out);
int mirge_reads_range_split(mirge_ctx* ctx, const mirge_reads* uniq, const uint64_t* splitters, int32_t n_parts, char* ascii_out,
                            int64_t* offsets_out, uint32_t* counts_out, int64_t* bounds_out);
int mirge_annotation_csv_device_sizes(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const int64_t* rows,
                                      int64_t n_rows, int32_t n_pass, const int32_t* col_of_pass, int32_t n_name_cols,
                                      const char* const* name_data, const int64_t* const* name_off, const int64_t* name_n,
                                      int64_t* bytes_out);
int mirge_annotation_csv_device_at(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const char* mapped_path,
                                   const char* unmapped_path, int64_t mapped_off, int64_t unmapped_off, const int64_t* rows,
                                   int64_t n_rows, int32_t n_pass, const int32_t* col_of_pass, int32_t n_name_cols,
                                   const char* const* name_data, const int64_t* const* name_off, const int64_t* name_n);

/* ---- per-position variant tally / A-to-I counting core (BASELINE config 5): replaces
 * align2TargetSeq / judgeAllign / A2IEditing / mismatchCountAnalysis (mirge2_tRF_a2i.py:246-518) and the membership
 * rules of a2i_editing (:988-1016) for the reads the cascade annotated to a miRNA in exact_pass / iso_pass.
 *   fam_of_ref[n_mirna]   family (merged miRNA name) of every reference of the miRNA library, -1 = none
 *   target_ascii/off      canonical sequence of each family (<org>_mirna_SNP_pseudo_<db>.fa), <= 32 nt
 *   retained[n reads]     the genome filter's answer per read in handle order (:1085-1096), NULL = every read
 *   freq[S]               1e6 / Filtered miRNA Reads per sample (an isomiR read is a member iff count*freq >= 1 somewhere)
 * out: fam_tables[5][n_fam][S] = n_seqs, seq_true, count_true, canon, kept_exact;
 *      census[n_fam][32][16][3][S] (position, target base * 4 + read base, variant raw / accepted / accepted+retained),
 *      read base != target base and position < len - 5 only;  A=0 C=1 G=2 T=3;
 *      diag_out/state_out[n reads] (may be NULL): diagonal of the alignment; 1 accepted, 0 rejected, -1 not a member.
 * Members of up to 64 nt are tallied (the isomiR policy annotates reads of up to 3 nt more than their miRNA: 35 nt for a
 * canonical sequence of 32).  Errors: -6 a canonical sequence of more than 32 nt, or a member of more than 64 nt (only a
 * policy that trims more can annotate one; nothing is left out of the tables in silence); -7 a canonical sequence with a
 * character other than A/C/G/T/U. */
#define MIRGE_TALLY_POSITIONS 32
int mirge_variant_tally(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, int32_t exact_pass,
                        int32_t iso_pass, const int32_t* fam_of_ref, int64_t n_mirna, const char* target_ascii,
                        const int64_t* target_off, int64_t n_fam, const uint8_t* retained, const double* freq,
                        int64_t* fam_tables, int64_t* census, int8_t* diag_out, int8_t* state_out);

/* ---- isomiR typing for the miRTop GFF3: replaces the per-read difflib.Differ diff and list
 * rewriting of create_gff (mirge/libs/summary.py:204-470) with one kernel.  For every read the cascade annotated in
 * exact_pass / iso_pass: the canonical sequence of its miRNA name (master_of_ref -> master tables), the precursor and
 * the canonical's position in it (what summary.py:147-186 looks up), and from those the record the reference prints:
 * type, precursor coordinates, Variant string, Cigar string.  slot_of_read[read] = row of records_out (-1: skip);
 * a record is MIRGE_ISO_RECORD_BYTES: int32 start, int32 end, uint8 kind (0 none, 1 ref_miRNA, 2 isomiR), uint8 pad,
 * uint16 variant length, uint16 cigar length, char text[320] (variant then cigar).                                 */
#define MIRGE_ISO_RECORD_BYTES 336
int mirge_isomir_type(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, int32_t exact_pass, int32_t iso_pass,
                      const int32_t* master_of_ref, int64_t n_mirna, const char* master_ascii, const int32_t* master_off,
                      const int32_t* pre_of_master, const int32_t* start0, int64_t n_master, const char* pre_ascii,
                      const int32_t* pre_off, int64_t n_pre, const int32_t* slot_of_read, int64_t n_rows, void* records_out);
/* the GFF3 file from those records (summary.py:60-64 header, :204 / :465 lines; UID = miRgeEssential.UID), formatted on
 * the host's cores; rows with kind 0 print nothing.  read_ascii/read_off, counts[.. * S] are per ROW when read_of_row is NULL;
 * otherwise they are the caller's whole table of n_reads unique reads and row k prints entry read_of_row[k] of it. */
int mirge_gff_write(const char* path, const char* head, const char* source, const void* records, int64_t n_rows,
                    const char* read_ascii, const int64_t* read_off, const uint32_t* counts, int32_t n_samples,
                    const int32_t* name_of_row, const char* name_data, const int64_t* name_off, int64_t n_names,
                    const int32_t* parent_of_row, const char* parent_data, const int64_t* parent_off, int64_t n_parents,
                    const int64_t* read_of_row, int64_t n_reads);
/* The same file from the DEVICE-resident run (round 6; what the CLI's -gff route calls): the rows are chosen (the exact-miRNA rows of
 * the mapped frame in frame order, then its isomiR rows: summary.py:50-60), typed, measured and formatted by kernels where the reads,
 * counts and annotation lie; only the file's text crosses PCIe.  order[k] = handle index of the read in row k of the run's frame
 * (mirge_collapse_order / mirge_collapse_order_sorted); the typing tables as mirge_isomir_type; name_of_ref / parent_of_ref
 * [n_mirna] index the two string tables (-1: the reference prints no line for reads of that name).  *n_lines_out = lines below
 * the head.  Replaces create_gff's per-read loop and its writes (mirge/libs/summary.py:204-470). */
int mirge_gff_write_device(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, int32_t exact_pass, int32_t iso_pass,
                           const int32_t* master_of_ref, int64_t n_mirna, const char* master_ascii, const int32_t* master_off,
                           const int32_t* pre_of_master, const int32_t* start0, int64_t n_master, const char* pre_ascii,
                           const int32_t* pre_off, int64_t n_pre, const int32_t* name_of_ref, const char* name_data,
                           const int64_t* name_off, int64_t n_names, const int32_t* parent_of_ref, const char* parent_data,
                           const int64_t* parent_off, int64_t n_parents, const int64_t* order, const char* path, const char* head,
                           const char* source, int64_t* n_lines_out);

/* ---- the A-to-I report's genome filter: replaces the two whole-genome runs
 * `bowtie <org>_genome -n 1 -f -a -3 2 SeqToMap.fasta` (mirge2_tRF_a2i.py:1056-1096) and `-n 0 ... SeqToJudge.fasta` (:1297-1316).
 * mirge_genome_create         the genome from ASCII references (<org>_genome.fa): anything but A/C/G/T is ambiguous.
 * mirge_genome_create_packed  the same from bowtie's own reference files, uploaded as they are: packed[n_packed] = .4.ebwt (2 bits
 *                             per base, base i at bits 2*(i & 3) of byte i >> 2), rec_off / rec_len / rec_first[n_rec] = the
 *                             .3.ebwt records (off ambiguous characters, then len bases; first: a new reference).  64-bit positions.
 * mirge_genome_destroy        (before its context)
 * mirge_genome_align_counts   out[n][3] = alignments of each query with 0, 1, 2 mismatches (saturating at UINT32_MAX) on both strands,
 *                             every valid alignment (-a): trim5 / trim3 bases cut (-5 / -3), at most n_mm mismatches in the first
 *                             min(seedlen, L) bases of the read's 5' end and maxtotal in all (-n; -e 70 with FASTA qualities: 2); an N in
 *                             a query mismatches everything, a window with an ambiguous base or across two references is invalid; a
 *                             query with L < 1 or L <= n_mm has none.  0 <= n_mm <= 2, maxtotal <= 2, L <= 64, seedlen >= 5 (bowtie's own floor for -l: every piece
 *                             of the seed holds a base); anything else is refused.  Restated from bowtie's documented -n policy
 *                             (parity unpinned).                                                                          */
typedef struct mirge_genome mirge_genome;
int mirge_genome_create(mirge_ctx* ctx, const char* ascii, const int64_t* offsets, int64_t n_refs, mirge_genome** out);
int mirge_genome_create_packed(mirge_ctx* ctx, const uint8_t* packed, int64_t n_packed, const uint64_t* rec_off,
                               const uint64_t* rec_len, const uint8_t* rec_first, int64_t n_rec, mirge_genome** out);
void mirge_genome_destroy(mirge_genome* genome);
int mirge_genome_align_counts(mirge_ctx* ctx, const mirge_genome* genome, const char* queries, const int64_t* offsets, int64_t n,
                              int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3, uint32_t* out);

/* ---- genome alignments with positions, and their clusters (the front half of -nmir, novel_mir.py:41-150,340-362)
 * mirge_genome_align_loci  every alignment mirge_genome_align_counts counts, as a record: the same predicate (one verify routine), plus
 *                          max_loci (bowtie -m: a query with more than max_loci valid alignments reports none; 0 = no cap) and norc
 *                          (forward strand only).  totals[n] = every query's valid alignments, capped or not.  The records
 *                          (mirge_loci_count / _fetch) are sorted by (reference, offset, query, strand with '+' = 0 first); offset is
 *                          0-based inside the reference, ambiguous stretches included (SAM POS - 1).  Queries are scanned in batches
 *                          of 2^20 against the one resident genome.
 * mirge_genome_align_loci_strata  the same with strata != 0: only the alignments of each query's best stratum (bowtie --best --strata
 *                          -a).  A stratum is the number of mismatches in the SEED (bowtie manual, -n mode), not in the whole read;
 *                          max_loci then counts the best stratum only (-m with --strata), totals[] stays every valid alignment and a
 *                          record's mm stays its total mismatch count.  strata = 0 is mirge_genome_align_loci.  Restated from the
 *                          manual, unpinned like the predicate.
 * mirge_loci_cluster       records sorted by (reference, offset) -> cluster[n] (-1: dropped) and the cluster table (caller's arrays
 *                          of n entries; *n_clusters filled) in (reference, strand, start) order.  Inside one (reference, strand) a
 *                          record joins iff offset + max(threshold, 1) <= the largest offset + qlen before it; ref_skip[r] != 0
 *                          drops reference r; minus_first_only != 0 keeps only the first minus-strand cluster of a reference, as
 *                          the reference does.  c_start 0-based, c_end exclusive, c_reads = sum of qcount.            */
typedef struct mirge_loci mirge_loci;
int mirge_genome_align_loci(mirge_ctx* ctx, const mirge_genome* genome, const char* queries, const int64_t* offsets, int64_t n,
                            int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3, int64_t max_loci,
                            int32_t norc, uint64_t* totals, mirge_loci** out);
int mirge_genome_align_loci_strata(mirge_ctx* ctx, const mirge_genome* genome, const char* queries, const int64_t* offsets, int64_t n,
                                   int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3, int64_t max_loci,
                                   int32_t norc, int32_t strata, uint64_t* totals, mirge_loci** out);
int64_t mirge_loci_count(const mirge_loci* loci);
int mirge_loci_fetch(const mirge_loci* loci, uint32_t* query, uint32_t* ref, uint64_t* off, uint8_t* strand, uint8_t* mm);
void mirge_loci_destroy(mirge_loci* loci);
int mirge_loci_cluster(mirge_ctx* ctx, int64_t n, const uint32_t* ref, const uint64_t* off, const uint8_t* strand,
                       const uint32_t* query, int64_t n_queries, const int32_t* qlen, const int64_t* qcount, int64_t n_refs,
                       const uint8_t* ref_skip, int32_t threshold, int32_t minus_first_only, int32_t* cluster,
                       int64_t* n_clusters, uint32_t* c_ref, uint8_t* c_strand, uint64_t* c_start, uint64_t* c_end,
                       int64_t* c_reads, uint32_t* c_members);

/* ---- cluster features (generate_featureFiles.py, readCluster.py, get_precursors): the reads of a sample stacked on their clusters
 * mirge_cluster_diagonals  per row (a read and the cluster it was aligned to; reads up to 64 nt, clusters up to 128 nt): diag = the best
 *                          ungapped local diagonal (cluster index - read index) under match +2 / mismatch -1, score = its score,
 *                          identity = equal bases over the WHOLE overlap of the two sequences on that diagonal, flag: bit 0 = score
 *                          <= 2 * min(L, C) - 20 (a gapped alignment at 20 per gap character could tie or win: the caller aligns that
 *                          row's cluster on the host), bit 1 = no positive score.  Equal scores: the diagonal whose end cell comes first
 *                          in the cluster, then first in the read.  A base that is not A/C/G/T matches nothing.
 * mirge_cluster_pileup     rows [row_start[k], row_start[k + 1]) are cluster k's.  head / tail[k] = the largest overhang of a read left /
 *                          right of the cluster; col_off[n_clusters + 1] = where cluster k's head + c_len + tail columns start in
 *                          tally[cap_cols][5] = the rows' counts summed per column and symbol in the order A, T, C, G, other.
 * mirge_genome_fetch       windows (reference, 0-based start, length) of the resident genome as ASCII at out + out_off[i] (out_off[n + 1],
 *                          out_off[i + 1] - out_off[i] = len[i]): 'N' where the genome holds no base, reverse-complemented when minus,
 *                          'U' for 'T' when rna.  The caller clamps the bounds; nothing is read past a reference's stretches. */
int mirge_cluster_diagonals(mirge_ctx* ctx, const char* reads, const int64_t* r_off, int64_t n_rows, const char* clusters,
                            const int64_t* c_off, int64_t n_clusters, const uint32_t* row_cluster, int32_t* diag, int32_t* score,
                            int32_t* identity, uint8_t* flag);
int mirge_cluster_pileup(mirge_ctx* ctx, const char* reads, const int64_t* r_off, int64_t n_rows, const int64_t* c_len,
                         const int64_t* row_start, int64_t n_clusters, const int32_t* diag, const int64_t* count, int32_t* head,
                         int32_t* tail, int64_t* col_off, int64_t* tally, int64_t cap_cols);
int mirge_genome_fetch(mirge_ctx* ctx, const mirge_genome* genome, int64_t n, const uint32_t* ref, const int64_t* start,
                       const int64_t* len, const uint8_t* minus, const uint8_t* rna, const int64_t* out_off, char* out);

/* ---- per-sample SAM alignments (`--sam-out`): the text the reference's -bam route hands to `samtools view` (manifoldAlign.py:12-64,
 * bamFmt.py:9-170, summary.py:841-880), one line per RAW read, formatted on the device and written chunk by chunk.
 * One call writes ONE sample's file: `header` (header_len bytes, verbatim), then for every class in class_pass[n_class] order (pass
 * numbers; at most 7; a pass not named writes nothing) the frame's rows of that pass in frame order (order[k] = handle index of the
 * read in row k), each with count c >= 1 in column `sample` as c lines `READ_k ...`, k = 0 .. c-1.  passes[n_pass] (n_pass >= the
 * result's) describe every named pass: its library, the -5 / -3 trim of its policy and the lift of its references to the genome:
 * chrom_of_ref[n_refs] indexes the chromosome strings (-1: reads of this reference write no line), minus[n_refs] != 0 = minus strand
 * (FLAG 16, SEQ reverse-complemented), seg_ptr[n_refs + 1] is a CSR into seg_s / seg_e (transcript coordinates, 1-based, inclusive)
 * and cds_lo / cds_hi (the two genome coordinates of the same segment as the header writes them).  *n_lines_out = lines below the
 * header, *n_bytes_out = their bytes.  Any failure returns an error code and removes the file.  Chunk and tile sizes:
 * MIRGE_SAM_CHUNK_BYTES / MIRGE_SAM_TILE_BYTES (README). */
typedef struct mirge_sam_pass {
    const mirge_lib* lib;
    int32_t trim5, trim3;
    int64_t n_refs;
    const int32_t* chrom_of_ref;
    const uint8_t* minus;
    const int64_t* seg_ptr;
    const int32_t* seg_s;
    const int32_t* seg_e;
    const int64_t* cds_lo;
    const int64_t* cds_hi;
    int64_t n_chrom;
    const char* chrom_data;
    const int64_t* chrom_off;
} mirge_sam_pass;
int mirge_sam_write_device(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const int64_t* order, int32_t sample,
                           const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass, const char* path,
                           const char* header, int64_t header_len, int64_t* n_lines_out, int64_t* n_bytes_out);

/* ---- per-sample sorted BAM and its index (`--sorted-bam`): the records of mirge_sam_write_device's file (same rows, same lift) as BAM v1,
 * sorted by (refID, pos, reverse flag) -- stably with respect to that file's row order, a row's copies in k order --, BGZF-compressed
 * and indexed, all produced on the device in one call.  `header` (header_len bytes) is the front of the uncompressed stream as the
 * caller built it: magic, l_text, text, n_ref and the n_ref references.  chrom_refid + chrom_refid_off[p] .. [p + 1] maps pass p's
 * chromosome indices (mirge_sam_pass.chrom_of_ref) to refIDs; -1 = no @SQ names it, an error when a kept row lies there.  Errors are
 * raised before anything is written: such a chromosome (named in the message), a position outside [0, 2^29), a QNAME beyond 254
 * characters.  *n_records_out = records, *n_stream_bytes_out = uncompressed bytes, *n_file_bytes_out = bytes of the .bam.
 * `threads` sizes the host pool of MIRGE_BAM_DEFLATE=host.  MIRGE_BAM_DEFLATE=device (the default) deflates every block on the device
 * with the fixed Huffman code or stores it; =dynamic adds a Huffman code built per block (BTYPE 10) and takes it where its member is
 * strictly smaller, so no member grows; =tight chooses among the same forms on the tokens of a closer parse (matches across the
 * threads' segments, record-aligned, repeat-distance and region candidates, one lazy step): no member larger than its stored form, no
 * promise per member against the other routes; =host sends the blocks through zlib on the host; any other value is an error.
 * MIRGE_BAM_BLOCK_BYTES / MIRGE_BAM_CHUNK_BLOCKS: README. */
int mirge_bam_write_device(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const int64_t* order, int32_t sample,
                           const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                           const int32_t* chrom_refid, const int64_t* chrom_refid_off, int32_t n_ref, const char* bam_path,
                           const char* bai_path, const char* header, int64_t header_len, int32_t threads, int64_t* n_records_out,
                           int64_t* n_stream_bytes_out, int64_t* n_file_bytes_out);

/* A test entry: the device's builder of the dynamic mode's code lengths alone (one workgroup).  counts[n_sym], 1 <= n_sym <= 288,
 * 1 <= max_bits <= 15, 2^max_bits >= n_sym -> lengths_out[n_sym]: 0 where the count is 0, none above max_bits; two or more used
 * symbols give a complete prefix code (of the Huffman optimum's cost whenever an optimal tree fits max_bits), one used symbol gets
 * length 1. */
int mirge_bam_huffman_probe(mirge_ctx* ctx, const uint32_t* counts, int32_t n_sym, int32_t max_bits, uint8_t* lengths_out);

/* ---- per-sample genome coverage as bedGraph (`--coverage`): depth per base from weighted intervals, as maximal runs of constant depth > 0.
 * mirge_coverage_runs          n intervals from host arrays: chrom_rank (0 .. 2^24 - 1), 0-based start, len >= 1, weight >= 1, minus;
 *                              depth(x) = the summed weight of the intervals that hold x, per strand when stranded != 0 (otherwise
 *                              every run has strand 0).  The runs (chromosome rank, [start, end), depth; abutting runs of equal depth are
 *                              one) arrive in file order -- plus strand first, then rank, then start -- in the caller's arrays of capacity
 *                              2 n; *n_runs_out = how many.  An interval outside the contract (end <= 2^31 - 1 included) fails the call;
 *                              2 n must stay below 2^31 - 16.
 * mirge_coverage_write_device  one sample's intervals are the rows of mirge_sam_write_device's file (same arguments up to n_pass): a row
 *                              with START, SEQ and count c is [START - 1, START - 1 + len(SEQ)) of weight c, minus iff FLAG 16.
 *                              chrom_rank + chrom_rank_off[p] .. [p + 1] maps pass p's chromosome indices to ranks 0 .. n_rank-1 (-1: the
 *                              caller's order does not hold the name, an error when a kept row lies there); rank_names /
 *                              rank_name_off[n_rank + 1] are the names in rank order.  The lines `chrom \t start \t end \t depth \n` go
 *                              to `path` (stranded == 0) or to `path` (plus) and `path_minus`.  Errors are raised before a file is
 *                              opened -- a chromosome without rank (named in the message), START < 1 or an end beyond 2^31 - 1 -- and
 *                              err_out[0..3] = kind (1 chromosome, 2 range), handle index of the unique read, pass, reference of the
 *                              first such row of the file; any failure leaves no file.  Outputs: intervals, their summed weight, lines
 *                              and bytes (both files together).  MIRGE_COV_CHUNK_BYTES / MIRGE_COV_TILE_BYTES: README. */
int mirge_coverage_runs(mirge_ctx* ctx, int64_t n, const int32_t* chrom_rank, const int64_t* start, const int32_t* len,
                        const uint32_t* weight, const uint8_t* minus, int32_t stranded, uint8_t* run_strand, int32_t* run_chrom,
                        int64_t* run_start, int64_t* run_end, int64_t* run_depth, int64_t* n_runs_out);
int mirge_coverage_write_device(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const int64_t* order, int32_t sample,
                                const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                                const int32_t* chrom_rank, const int64_t* chrom_rank_off, int32_t n_rank, const char* rank_names,
                                const int64_t* rank_name_off, int32_t stranded, const char* path, const char* path_minus,
                                int64_t* n_intervals_out, int64_t* weight_out, int64_t* n_lines_out, int64_t* n_bytes_out,
                                int64_t* err_out);

/* ---- the runs of `--coverage` as bigWig (`--coverage-bigwig`; the format: mirge3_amd/bigwig.py): one file per strand, written to
 * `<path>.tmp` and renamed when every file of the call is whole; any failure leaves no file.
 * mirge_bigwig_from_intervals  host intervals as in mirge_coverage_runs.  rank_names / rank_name_off[n_rank + 1]: ALL chromosome names
 *                              in rank order (n_rank >= 1), chrom_size[rank] <= 2^32 - 1, chrom_id[rank] = the name's position among
 *                              the names sorted by bytes (checked).  stats_out[16 f + ..] of file f: sections, items, zoom levels,
 *                              bytes, the largest depth, then the records of every kept level.  A run that ends beyond its
 *                              chromosome's size fails the call with err_out = {3, rank, end, size}.
 * mirge_bigwig_write_device    the resident run: the arguments of mirge_coverage_write_device up to rank_name_off, then the sizes and
 *                              ids as above; err_out kinds 1 and 2 as there, 3 as above.
 * MIRGE_BW_SECTION_ITEMS (1 .. 1024), MIRGE_BW_ZOOM_BASE (default 64), MIRGE_BW_DEFLATE (device | none), MIRGE_BW_CHUNK_BYTES: README. */
int mirge_bigwig_from_intervals(mirge_ctx* ctx, int64_t n, const int32_t* chrom_rank, const int64_t* start, const int32_t* len,
                                const uint32_t* weight, const uint8_t* minus, int32_t stranded, int32_t n_rank, const char* rank_names,
                                const int64_t* rank_name_off, const int64_t* chrom_size, const int32_t* chrom_id, const char* path,
                                const char* path_minus, int64_t* stats_out, int64_t* err_out);
int mirge_bigwig_write_device(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const int64_t* order, int32_t sample,
                              const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                              const int32_t* chrom_rank, const int64_t* chrom_rank_off, int32_t n_rank, const char* rank_names,
                              const int64_t* rank_name_off, const int64_t* chrom_size, const int32_t* chrom_id, int32_t stranded,
                              const char* path, const char* path_minus, int64_t* stats_out, int64_t* err_out);

/* ---- `--bgzf-out`: the text of `--sam-out` and `--coverage` as BGZF, deflated on the device where it is produced (the format, the
 * member rule and the `.gzi` layout: mirge3_amd/bgzf.py).  The stream is cut into blocks of block_bytes (64 .. 65280; <= 0:
 * MIRGE_BGZF_BLOCK_BYTES, default 65280); the file is a function of the stream and the block size alone.  Every file is written as
 * `<path>.tmp` and renamed when all files of the call are whole; any failure leaves no file.  MIRGE_BGZF_DEFLATE=device (the default) |
 * host (zlib level 6 on MIRGE_GZ_THREADS threads); any other value fails the call before a file is opened.
 * stats_out[8] per file: file bytes, members stored, fixed, dynamic, members, stream bytes, 0, 0.
 * mirge_bgzf_write                  n bytes from the host -> `path` and its index `gzi_path` (MIRGE_BGZF_CHUNK_BYTES: bytes per chunk).
 * mirge_sam_write_device_bgzf       mirge_sam_write_device's arguments; `path` is the .sam.gz (the header is the front of the stream).
 * mirge_coverage_write_device_bgzf  mirge_coverage_write_device's arguments; each strand's file is a stream of its own; stats_out[16]. */
int mirge_bgzf_write(mirge_ctx* ctx, const uint8_t* bytes, int64_t n, int64_t block_bytes, const char* path, const char* gzi_path,
                     int64_t* stats_out);
int mirge_sam_write_device_bgzf(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const int64_t* order, int32_t sample,
                                const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass, const char* path,
                                const char* header, int64_t header_len, int64_t* n_lines_out, int64_t* n_bytes_out, const char* gzi_path,
                                int64_t block_bytes, int64_t* stats_out);
int mirge_coverage_write_device_bgzf(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const int64_t* order, int32_t sample,
                                     const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                                     const int32_t* chrom_rank, const int64_t* chrom_rank_off, int32_t n_rank, const char* rank_names,
                                     const int64_t* rank_name_off, int32_t stranded, const char* path, const char* path_minus,
                                     int64_t* n_intervals_out, int64_t* weight_out, int64_t* n_lines_out, int64_t* n_bytes_out,
                                     int64_t* err_out, const char* gzi_path, const char* gzi_path_minus, int64_t block_bytes,
                                     int64_t* stats_out);

/* ---- the sequence work behind the tRNA fragment report (the reference's -trf: summary.py:1060-1220, mirge2_tRF_a2i.py:22-62)
 * mirge_trf_hits_run  every best-stratum alignment (bowtie -a --best --strata) of the tRNA reads rows[n_rows] (handle indices of `uniq`;
 *                     a record's row is the index INTO rows).  A read the cascade gave to mature_pass: every forward window of
 *                     mature_lib whose total mismatches equal the read's stratum (the result's mm; N in the read is a mismatch, a
 *                     window over a separator or a reference N is no hit).  A read of primary_pass: every exact window of the read
 *                     without its T{3,}$ run in primary_lib.  Both policies are -v policies without trims.  The probe tables the rows
 *                     need are built on first use.  anticodon[mature references] = 0-based start of the anticodon.  Records
 *                     (mirge_trf_hits_count / _fetch / _destroy) are sorted by (row, ref, off), every window once: ref / off = reference
 *                     and 0-based offset in the class's library, mm = the stratum, cls = 0 mature / 1 primary, type = trfTypes
 *                     (summary.py:649-674) decided by the class: 0 tRF-whole, 1 5'-half, 2 5'-tRF, 3 3'-half, 4 3'-tRF, 5 i-tRF, 6 tRF-1.
 * mirge_trf_assign    assign_cluster / getDistance2 for n_rows report rows: read[] = handle index of the row's read, tref[] = the row's
 *                     reference as an index into ref_ptr[n_tref + 1] (a CSR over the n_trf predefined tRFs; -1: the reference has none),
 *                     start[] = 1-based start.  tRF k: its dashed string str[str_off[k] .. str_off[k + 1]) as text, its coordinate()
 *                     pair c_start / c_end, and rank = the rank of its cluster name in string order.  dist[] / trf[] = the minimum of
 *                     (distance, rank) and its tRF index; 100 / -1 for a reference without tRFs.  Distance = |start difference| + |end
 *                     difference| (the row's end coordinate is start - 1 + len(read), T run included) + positions where both strings
 *                     hold a letter and differ (as text: N equals only N) + every letter of the row at or beyond len(string). */
typedef struct mirge_trf_hits mirge_trf_hits;
int mirge_trf_hits_run(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, int32_t mature_pass, const mirge_lib* mature_lib,
                       const mirge_policy* mature_pol, int32_t primary_pass, const mirge_lib* primary_lib, const mirge_policy* primary_pol,
                       const int64_t* rows, int64_t n_rows, const int32_t* anticodon, mirge_trf_hits** out);
int64_t mirge_trf_hits_count(const mirge_trf_hits* hits);
int mirge_trf_hits_fetch(const mirge_trf_hits* hits, uint32_t* row, uint32_t* ref, int32_t* off, uint8_t* mm, uint8_t* cls, uint8_t* type);
void mirge_trf_hits_destroy(mirge_trf_hits* hits);
int mirge_trf_assign(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, int64_t n_rows, const int64_t* read,
                     const int32_t* tref, const int32_t* start, int64_t n_tref, const int64_t* ref_ptr, int64_t n_trf,
                     const int64_t* str_off, const char* str, const int32_t* c_start, const int32_t* c_end, const int32_t* rank,
                     int32_t* dist, int32_t* trf);
/* out[n_rows][n_samples] = the count matrix of `uniq` for the reads rows[] alone (the report's rows: no fetch of the whole matrix) */
int mirge_trf_row_counts(mirge_ctx* ctx, const mirge_reads* uniq, const int64_t* rows, int64_t n_rows, uint32_t* out);

/* ---- density-peak clustering of the reads stacked on a tRNA (--trf-clusters: getDistance / local_density / min_distance and the
 * centre / halo loop of trna_deliverables, mirge2_tRF_a2i.py:122-207, 776-839)
 * mirge_trf_cluster   n_grp groups of points as a CSR grp_ptr[n_grp + 1]; a point = a row of <sample>.aligned_tRFs.report: read[] = the
 *                     handle index in `uniq`, off[] = its 0-based offset in the template, rp100k[] = its RP100K as the report prints
 *                     it; tlen[n_grp] = the template's length (at most 256, or the call fails: "a template of N columns is longer than
 *                     256"; off + len(read) <= tlen).  gauss[n_gauss] = exp(-(d / 3) ** 2) for d = 0 .. n_gauss - 1, n_gauss >= 2 * the
 *                     longest template + 1: the device evaluates no exp.  Distance of two points = |start difference| + |end
 *                     difference| + columns where both hold a letter and the letters differ (N equals only N), from the packed words;
 *                     it is recomputed wherever it is needed and no n x n matrix exists.  Per point, 1-based within its group:
 *                     rho = float32 of (sum over j != i, ascending, of gauss[d] * rp100k[j], + rp100k[i]) in doubles, product and sum
 *                     rounded separately; order = the 0-based position in the order ascending (-rho, index); delta / nneigh = the
 *                     nearest point ahead in that order, of equal distances the last (nneigh 0 and delta = the largest other delta, or
 *                     0, for the first); cl = the cluster (-1: none), halo = cl or 0.  Per group nclust, and centre[grp_ptr[g] + k] =
 *                     the centre of cluster k + 1 (0 behind the last).  Centres: rho >= 5 and delta >= 8, else the densest point when
 *                     every delta <= 8 and its rho >= 5. */
int mirge_trf_cluster(mirge_ctx* ctx, const mirge_reads* uniq, int64_t n_grp, const int64_t* grp_ptr, const int64_t* read, const int32_t* off,
                      const double* rp100k, const int32_t* tlen, int64_t n_gauss, const double* gauss, float* rho, float* delta,
                      int32_t* nneigh, int32_t* order, int32_t* cl, int32_t* halo, int32_t* nclust, int32_t* centre);

/* ---- per-sample read QC (--read-qc; mirge3_amd/readqc.py holds the specification)
 * mirge_qc            the accumulator of ONE sample: the 64-bit tables of the `raw` and the `trimmed` view in device memory, alive across the
 *                     pieces of a streamed sample.  Integer sums only: the tables do not depend on how the sample was cut into pieces.
 * mirge_reads_parse_trim_qc   mirge_reads_parse_trim (trim may be NULL) that also adds the text's records to `qc` (NULL: exactly
 *                     mirge_reads_parse_trim).  raw = every record's sequence line (a trailing '\r' stripped); trimmed = the read after the
 *                     LAST modifier, once per record whatever count_per_modifier says, if it has at least min_len letters.  MIRGE_QC_FORM =
 *                     pos (a lane per position) | read (a lane per read, the default): two forms of the text histogram, the same tables.
 * mirge_qc_fetch      tables[2][MIRGE_QC_VIEW_WORDS = 92467] (raw, then trimmed), each view: [0..7] the scalars reads, bases, reads_with_N,
 *                     empty_reads, qual_clamped, qual_length_mismatch, 0, 0; [8 ..] length[65536]; base[257][5] (letters A C G T N; row 256:
 *                     positions of 256 and more); qual[257][94]; meanq[94]; gc[101]; first[257][5] (row = min(length, 256)).
 *                     *has_qual = 1 when a FASTQ piece went in (else the quality tables are zero and mean nothing).
 * mirge_qc_class_profile      out[n_samples][n_pass + 1][257][5][2]: per sample, class (the pass that annotated the read; n_pass: none),
 *                     min(length, 256) and first letter (an empty read: N) the sum of the unique reads' counts and the number of unique
 *                     reads with a count > 0. */
typedef struct mirge_qc mirge_qc;
int mirge_qc_create(mirge_ctx* ctx, mirge_qc** out);
void mirge_qc_destroy(mirge_qc* qc);
int mirge_reads_parse_trim_qc(mirge_ctx* ctx, const char* text, int64_t nbytes, int32_t format, int32_t min_len, const mirge_trim* trim,
                              mirge_qc* qc, mirge_reads** out, int64_t* n_records);
int mirge_qc_fetch(mirge_ctx* ctx, const mirge_qc* qc, int64_t* tables, int32_t* has_qual);
int mirge_qc_class_profile(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, int32_t n_pass, int64_t* out);

/* ---- the trimmed reads of a sample as FASTQ / FASTA / one sequence per line (--trimmed-out; mirge3_amd/trimmed_out.py holds the specification)
 * mirge_fqout         the writer of ONE sample, alive across the pieces of a streamed sample: `path` (written as `<path>.tmp`), and with
 *                     gzi_path != NULL `path` is a BGZF file (mirge3_amd/bgzf.py) and gzi_path its block index; block_bytes <= 0:
 *                     MIRGE_BGZF_BLOCK_BYTES.  A wrong MIRGE_BGZF_BLOCK_BYTES / MIRGE_BGZF_DEFLATE fails the create.
 * mirge_reads_parse_trim_out  mirge_reads_parse_trim_qc (qc may be NULL) that also appends the piece's part of the stream S to `fq` (NULL:
 *                     exactly mirge_reads_parse_trim_qc): in file order every record whose read after the LAST modifier has at least min_len
 *                     letters, as  H \n S \n + \n Q \n  (format 1),  H \n S \n  (2) or  S \n  (3); H the header line and S the read
 *                     verbatim, Q the same slice of the quality line, a trailing '\r' stripped from each.  A quality line that is not as long
 *                     as its sequence line fails the call (`--trimmed-out: ...`) before the piece writes anything; a piece writes only after
 *                     its reads were packed without error.  A failed call leaves no file of the sample, and the writer takes no more pieces.
 *                     S does not depend on how the sample was cut into pieces, nor on MIRGE_FQ_CHUNK_BYTES (default 32 MiB) or
 *                     MIRGE_FQ_TILE_BYTES (a multiple of 16, at most 16384).  BGZF: member b holds S[b * B, (b + 1) * B).
 * mirge_fqout_finish  the last, short member, the EOF block and the .gzi (BGZF); the files are renamed to their names.
 *                     stats_out[8]: records, written, stream bytes, file bytes, members, members stored, fixed, dynamic.
 * mirge_fqout_destroy without finish: the .tmp files are removed. */
typedef struct mirge_fqout mirge_fqout;
int mirge_fqout_create(mirge_ctx* ctx, const char* path, const char* gzi_path, int64_t block_bytes, mirge_fqout** out);
int mirge_reads_parse_trim_out(mirge_ctx* ctx, const char* text, int64_t nbytes, int32_t format, int32_t min_len, const mirge_trim* trim,
                               mirge_qc* qc, mirge_fqout* fq, mirge_reads** out, int64_t* n_records);
int mirge_fqout_finish(mirge_ctx* ctx, mirge_fqout* fq, int64_t* stats_out);
void mirge_fqout_destroy(mirge_fqout* fq);

/* ---- unannotated reads' nearest hairpin by edit distance (--unmapped-nearest; mirge3_amd/nearest.py holds the specification)
 * mirge_nearest_scan  queries q[n_q] and targets t[n_t] as ASCII + offsets (n + 1 each).  For EVERY query: D (the smallest unit-cost edit
 *                     distance to a non-empty substring of a target; -1 for a query shorter than 12 or longer than 64 letters, or when
 *                     no target has a base), the target of lowest index that reaches it, there the smallest end e and for it the largest
 *                     start s (0-based, h[s:e]); hairpin = s = e = -1 where D = -1.  No K and no cap.  Letters match iff equal and one
 *                     of A C G T.  The kernels are the run's.  Limits: 2^24 targets, fewer than 2^32 - 16 target bases in all,
 *                     fewer than 2^31 - 16 queries.  MIRGE_NEAR_CHUNK_BASES (1 .. 4096, default 4096): bases per workgroup's run of
 *                     whole targets (a longer target is a run of its own); MIRGE_NEAR_FORCE64=1: every query in the 64-bit instance.
 *                     Neither changes a result.
 * mirge_nearest_unmapped  the same over the rows of `uniq` that `res` left at MIRGE_NO_PASS and that are 12 .. 64 nt long; kept are the
 *                     rows with D <= min(K, length / 8), 1 <= K <= 8.  mirge_nearest_count / _fetch: the kept rows in ascending handle
 *                     index: row, D, hairpin, s, e.  mirge_nearest_stats: stats_out[5] = unannotated rows, of them too short, too long,
 *                     considered, kept. */
typedef struct mirge_nearest mirge_nearest;
int mirge_nearest_scan(mirge_ctx* ctx, const char* q_text, const int64_t* q_off, int64_t n_q, const char* t_text, const int64_t* t_off,
                       int64_t n_t, int32_t* dist, int32_t* hairpin, int32_t* start, int32_t* end);
int mirge_nearest_unmapped(mirge_ctx* ctx, const mirge_reads* uniq, const mirge_result* res, const char* t_text, const int64_t* t_off,
                           int64_t n_t, int32_t K, mirge_nearest** out);
int64_t mirge_nearest_count(const mirge_nearest* hits);
int mirge_nearest_fetch(const mirge_nearest* hits, uint32_t* row, int32_t* dist, int32_t* hairpin, int32_t* start, int32_t* end);
int mirge_nearest_stats(const mirge_nearest* hits, int64_t* stats_out);
void mirge_nearest_destroy(mirge_nearest* hits);

/* ---- measurement (bench.py): HIP events on the ctx stream ---- */
int mirge_ctx_timer_start(mirge_ctx* ctx);
int mirge_ctx_timer_stop(mirge_ctx* ctx, double* ms_out);
int mirge_ctx_profile_enable(mirge_ctx* ctx, int32_t on);
/* record only launches whose name contains `substr` (NULL or "" = every launch) */
int mirge_ctx_profile_only(mirge_ctx* ctx, const char* substr);
/* on = 0: the bracketed cascade launches are timed but the reads handed to each pass (their "units") are no longer read
 * back -- a device-to-host copy per call on the critical path (bench.py's timed region: the units of the same batch are
 * known from its profiled warm-up steps) */
int mirge_ctx_profile_units(mirge_ctx* ctx, int32_t on);
int mirge_ctx_profile_reset(mirge_ctx* ctx);
int32_t mirge_ctx_profile_count(mirge_ctx* ctx);
int mirge_ctx_profile_get(mirge_ctx* ctx, int32_t i, char* name_out, int32_t name_cap,
                          int64_t* launches, double* total_ms, double* units);

#ifdef __cplusplus
}
#endif
#endif
