/*
 * bwtmi.h -- C ABI of libbwtmi.so, the MI355X-native (gfx950) BWT/FM-index and
 * tandem-repeat engine behind the `bwt.py` drop-in surface.
 *
 * The reference (wyim-pgl/bwt-algorithm, bwt.py) is pure Python and has no
 * FFI; its "interface" is the Python names listed below.  Each entry point
 * here replaces the body of one of those names; the Python host
 * (bwt-algorithm_amd/bwtmi) keeps the names and binds these symbols with
 * ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, a negative BWTMI_E* code on error;
 *     bwtmi_last_error() returns the thread-local message of the last error.
 *   - inputs are caller-owned and only borrowed for the duration of a call;
 *     outputs allocated by the library are released with bwtmi_free() or the
 *     matching *_free().
 *   - one bwtmi_ctx per device; calls on one ctx are serialised by the caller.
 *     HIP is not fork-safe: never fork() after bwtmi_open().
 *   - there is no CPU fallback: without a usable gfx950 device bwtmi_open()
 *     fails with BWTMI_E_NODEVICE.
 */
#ifndef BWTMI_H
#define BWTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BWTMI_OK 0
#define BWTMI_E_ARG (-1)
#define BWTMI_E_NODEVICE (-2)
#define BWTMI_E_HIP (-3)
#define BWTMI_E_NOMEM (-4)
#define BWTMI_E_STATE (-5)
#define BWTMI_E_IO (-6)

typedef struct bwtmi_ctx bwtmi_ctx;
typedef struct bwtmi_index bwtmi_index;
typedef struct bwtmi_job bwtmi_job;

/* ------------------------------------------------------------ context */
const char *bwtmi_last_error(void);
/* "bwtmi 0.5 (gfx950) src <sha256>": the sources the library was built from */
const char *bwtmi_version(void);
/* sha256 (hex) of the csrc sources (.cpp, .h, .hip) and include/bwtmi.h, concatenated in
 * byte order of their paths, computed by the Makefile at build time: a test
 * or launcher compares it with the tree it runs from (bwtmi._lib.check_build) */
const char *bwtmi_source_hash(void);
int bwtmi_device_count(int *count);
int bwtmi_open(int device, bwtmi_ctx **out);
int bwtmi_close(bwtmi_ctx *ctx);
/* Host placement, asked for explicitly (the CLI, bench.py and the rank
 * launcher do; bwtmi_open never does unless BWTMI_NUMA_BIND=1): on=1 moves
 * this process's host work -- the calling thread now, the library's worker
 * threads at their next parallel region -- onto the CPUs of the NUMA node of
 * ctx's GPU; on=0 restores the affinity the binding replaced.  *changed = 1
 * when the placement changed.  Local rank r (LOCAL_RANK / LOCAL_WORLD_SIZE)
 * drives device r mod (visible devices); the ranks whose GPUs share this
 * node decide whether one hardware thread per core is taken.  A second
 * context on another node leaves the first binding in place. */
int bwtmi_bind_host(bwtmi_ctx *ctx, int on, int *changed);
/* The CPU set bwtmi_bind_host would choose, without changing anything: sysfs
 * read under `sysroot` ("/sys" on a host; a faked tree in the tests), local
 * rank `local_rank` of the ranks whose GPUs have the comma-separated PCI
 * addresses `rank_pci` (rank order), `threads` host threads per rank, `smt`
 * = keep sibling hardware threads, `allowed` = the process's affinity as a
 * cpulist.  out = the chosen cpulist ("" = no binding); *node = this GPU's
 * NUMA node, *ranks_on_node = local ranks whose GPUs sit on it. */
int bwtmi_host_binding_plan(const char *sysroot, int local_rank, const char *rank_pci, int threads, int smt,
                            const char *allowed, char *out, int64_t cap, int *node, int *ranks_on_node);
/* Run-time switches (INTEGRATION.md "Run-time switches"): BWTMI_<NAME> read
 * once from the environment; get/set in-process by NAME (with or without the
 * BWTMI_ prefix).  Unknown names: BWTMI_E_ARG.  bwtmi_knob_names(): all names,
 * comma-separated. */
/* roctx ranges (rocprofv3 --marker-trace): the library opens "bwtmi:<stage>"
 * around load, upload, scan, index, merge, refine..filter, compounds, format,
 * write and index_wait; a host application can nest its own with these. */
int bwtmi_trace_push(const char *name);
int bwtmi_trace_pop(void);
int bwtmi_knob_set(const char *name, int64_t value);
int bwtmi_knob_get(const char *name, int64_t *value);
int bwtmi_knob_default(const char *name, int64_t *value);
const char *bwtmi_knob_names(void);
void bwtmi_free(void *p);
/* time (ms) of the kernels of the last call on ctx, measured with HIP events
 * on the ctx stream: [0]=total device, [1]=dominant kernel, [2]=its launches */
int bwtmi_last_timing(bwtmi_ctx *ctx, double *out3);

/* per-kernel HIP-event timing on the ctx stream: enable=1 starts collecting,
 * the call writes "name ms launches\n" lines of everything collected so far
 * into out (cap bytes, NUL-terminated) and resets when reset=1 */
int bwtmi_kernel_stats(bwtmi_ctx *ctx, int enable, int reset, char *out, int64_t cap);
/* time only the launches named `name` (NULL or "": every launch); the others
 * then run without event records between them */
int bwtmi_kernel_stats_filter(bwtmi_ctx *ctx, const char *name);

/* ------------------------------------------------------------ strict scan
 * Replaces Tier2LCPFinder.find_long_unit_repeats_strict (bwt.py:1891-2001),
 * as called by _process_chromosome_worker (bwt.py:3103-3106).
 * seq: ASCII bases of one (trimmed) contig; a single trailing '$' is ignored
 * (bwt.py:1915-1916).  Hits come out in the reference's emission order
 * (unit_len descending, start ascending).  prim_len = smallest_period_str of
 * the first unit (bwt.py:1956); copies = count after primitive reduction
 * (bwt.py:1957-1961).  max_mismatch 0 is the CLI value; > 0 compares adjacent
 * L-blocks by Hamming distance <= max_mismatch (bwt.py:1929-1944, library calls). */
typedef struct {
    int64_t start;
    int64_t end;
    int32_t unit_len;
    int32_t prim_len;
    int64_t copies;
} bwtmi_hit;

int bwtmi_strict_scan(bwtmi_ctx *ctx, const uint8_t *seq, int64_t n, int32_t min_unit,
                      int32_t max_unit, int32_t max_mismatch, int32_t min_copies,
                      bwtmi_hit **hits, int64_t *nhits);

/* The device screen (nested.hip) on a caller's hit list, as the scan runs it on
 * its own hits: nested suppression, (start, end, prim desc) order, dedup, then
 * the drop (drop != 0 and BWTMI_SCREEN_DROP) and the cut bits.
 * Every hit must satisfy 0 <= start < end <= text_len and prim_len >= 1
 * (unit_len and copies are not read); min_copies >= 1; BWTMI_E_ARG otherwise,
 * before anything reaches the device.
 * maxlen: the longest span if known, -1 to reduce it on the device.
 * out: malloc'd, 4 int64 per surviving hit {start, len, prim, cut}; free with bwtmi_free. */
int bwtmi_screen_hits(bwtmi_ctx *ctx, const bwtmi_hit *hits, int64_t n, int64_t text_len,
                      int32_t min_copies, int32_t drop, int64_t maxlen,
                      int64_t **out, int64_t *nout);

/* ------------------------------------------------------------ device primitives
 * The radix sort and the exclusive scans every device stage is built on
 * (radix.hip), run on a caller's host arrays (tests, embedders): the arrays are
 * copied to device buffers of the entry's own, the primitive runs on the
 * context's stream exactly as the library's stages call it, and the results are
 * copied back.  Not in the reference.
 *
 * bwtmi_radix_sort: the stable LSD sort of n keys (and their values) by the
 * key bits [bit0, bit1), 8 bits per pass, in place in the caller's arrays.
 *   kind   K64V64  uint64 keys, uint64 values       K32V32    uint32 / uint32
 *          K64V32  uint64 keys, uint32 values       K16V32    uint16 / uint32
 *          K64     uint64 keys alone (vals is not read and may be NULL)
 *          PASS_K32  one out-of-place pass over uint32 keys and values by the
 *                  digit at bit0 (bit1 = bit0 + 8): the pass's outputs come back
 *                  in keys / vals, and the call fails with BWTMI_E_STATE if the
 *                  pass changed its inputs on the device.
 *   skew   0..15: the device arrays start that many elements past a 16-byte
 *          aligned address (0: the histogram's 16-byte loads; otherwise, unless
 *          skew elements are a multiple of 16 bytes, its scalar loads).
 *   stable pairs of equal digits keep their order: the result is
 *          keys[order], vals[order] with order = the stable argsort of
 *          (keys >> bit0) & (2^(bit1 - bit0) - 1); bits outside the range ride along.
 *   errors BWTMI_E_ARG before anything reaches the device, the arrays
 *          untouched: an unknown kind, n < 0 or n >= 2^32, a null array with
 *          n > 0, bit0 < 0, bit1 above the key width, bit0 >= bit1, a range that
 *          is not a whole number of 8-bit digits (the library's own callers get
 *          such a range rounded up; this entry refuses it), skew outside 0..15.
 *          BWTMI_E_STATE: a device check (BWTMI_DEVICE_CHECKS) fired, or bytes
 *          next to the device arrays were written.  n = 0 is legal. */
#define BWTMI_SORT_K64V64 0
#define BWTMI_SORT_K64V32 1
#define BWTMI_SORT_K64 2
#define BWTMI_SORT_K32V32 3
#define BWTMI_SORT_K16V32 4
#define BWTMI_SORT_PASS_K32 5
int bwtmi_radix_sort(bwtmi_ctx *ctx, int32_t kind, void *keys, void *vals, int64_t n, int32_t bit0,
                     int32_t bit1, int32_t skew);
/* bwtmi_exclusive_scan: out[r * stride + i] = in[r * stride] + ... + in[r * stride + i - 1]
 * for each of `rows` rows of n elements, `stride` elements apart (rows = 1:
 * stride is not read).  in and out hold (rows - 1) * stride + n elements.
 *   kind     U32: uint32 sums mod 2^32, any number of rows (the single-pass
 *            look-back scan).  I64: int64 sums, rows = 1 (the three-launch scan).
 *   in_place != 0: the scan runs with out == in on the device.  Otherwise the
 *            device output array starts as a copy of the caller's `out`, so the
 *            elements between rows come back as they were, and the call fails
 *            with BWTMI_E_STATE if the scan changed its input.
 *   skew     0..15: as above, for the first row's base on the device.
 *   epoch    0: nothing.  Otherwise the context's look-back epoch (the tag that
 *            tells one launch's published tile sums from an earlier launch's,
 *            drawn per launch, wrapping at 2^30 with the sums cleared) is set to
 *            this value before the scan, so a test can reach the wrap.  Accepted
 *            only when it is above the context's current epoch and below 2^30:
 *            the epoch never moves backwards, because an epoch used twice
 *            without the clear between could match a stale sum.
 *   errors   BWTMI_E_ARG before anything reaches the device, `out` untouched:
 *            an unknown kind, n, rows - 1 or stride negative (or n, stride >=
 *            2^32, rows > 65536), a null array with n > 0, rows > 1 with I64 or
 *            with stride < n, skew outside 0..15, an epoch not accepted.
 *            n = 0 is legal. */
#define BWTMI_SCAN_U32 0
#define BWTMI_SCAN_I64 1
int bwtmi_exclusive_scan(bwtmi_ctx *ctx, int32_t kind, const void *in, void *out, int64_t n, int32_t rows,
                         int64_t stride, int32_t skew, int32_t in_place, int64_t epoch);

/* ------------------------------------------------------------ FM index
 * Replaces BWTCore.__init__ (bwt.py:106-136): suffix array (212-264), BWT
 * (266-274), C table (276-286), Occ checkpoints (288-326), sampled SA
 * (328-333) and the 8-mer hash (138-171).  text includes the sentinel, exactly
 * as the reference receives it (seq + '$'). */
#define BWTMI_INDEX_NO_KMER 1u
/* BWTMI_INDEX_REVERSE: after the forward build, also build a second index over
 * R = reverse(T[0, n-1)) + T[n-1] on the device, from the resident text, with
 * the same sample rates and no k-mer table; it is held inside the index and
 * released by bwtmi_index_free.  bwtmi_index_smem_long_batch needs it; nothing
 * else reads it, and without the flag the build and every getter are as they
 * were (with it the getters still return the forward index).  Requires n >= 1
 * and that T[n-1] occurs exactly once in T (seq + '$' always does), else
 * BWTMI_E_ARG and nothing is built.  The build runs the suffix sort twice, so
 * its time roughly doubles; of the reverse index only the rank structures are
 * kept (BWT, Occ checkpoints, packed blocks): about 1.7 n bytes more on an ACGT
 * text at the default rates, beside a forward index of about 6.8 n without its
 * k-mer table.  While the reverse build runs, its text, suffix array and
 * samples (5.1 n more) are resident too, so the build's peak device memory is
 * nearly twice the forward index's. */
#define BWTMI_INDEX_REVERSE 2u

int bwtmi_index_build(bwtmi_ctx *ctx, const uint8_t *text, int64_t n, int32_t sa_sample,
                      int32_t occ_sample, uint32_t flags, bwtmi_index **out);
int bwtmi_index_free(bwtmi_index *idx);
/* 1 when the index was built with BWTMI_INDEX_REVERSE, else 0 (NULL: 0) */
int bwtmi_index_has_reverse(const bwtmi_index *idx);
int64_t bwtmi_index_size(const bwtmi_index *idx);
int bwtmi_index_get_sa(const bwtmi_index *idx, int32_t *sa /* n */);
int bwtmi_index_get_bwt(const bwtmi_index *idx, uint8_t *bwt /* n */);
/* totals[256] and cumulative C[256] over byte values (absent bytes: total 0) */
int bwtmi_index_get_counts(const bwtmi_index *idx, int64_t *totals, int64_t *C);
/* checkpoints of one byte code; length = 1 + n/occ + (n%occ != 0) */
int64_t bwtmi_index_occ_len(const bwtmi_index *idx);
int bwtmi_index_get_occ(const bwtmi_index *idx, uint8_t code, int32_t *cp);
/* sampled SA (bwt.py:328-333): values SA[i] for i = 0, s, 2s, ... */
int64_t bwtmi_index_sampled_len(const bwtmi_index *idx);
int bwtmi_index_get_sampled(const bwtmi_index *idx, int32_t *vals);
/* 8-mer hash as CSR: offsets[65537], positions[offsets[65536]] */
int64_t bwtmi_index_kmer_count(const bwtmi_index *idx);
int bwtmi_index_get_kmer(const bwtmi_index *idx, int64_t *offsets, int32_t *positions);
/* Kasai LCP over the index text (bwt.py:56-95, 2108-2116), int32[n] */
int bwtmi_index_lcp(bwtmi_ctx *ctx, bwtmi_index *idx, int32_t *lcp);
/* Library finders of Tier2LCPFinder over an index (not on the CLI path). */
typedef struct {
    int32_t min_period;        /* Tier2LCPFinder(min_period=1, max_period=1000, max_short_motif=9) */
    int32_t max_period;
    int32_t max_short_motif;
    int32_t min_copies;        /* self.min_copies = 3 (bwt.py:1880) */
    int32_t min_array_length;  /* 6 (bwt.py:1881) */
    int32_t allow_mismatches;
    double min_entropy;        /* 1.0 (bwt.py:1882) */
} bwtmi_lib_params;
/* _detect_lcp_plateaus over the index's Kasai LCP (bwt.py:2118-2145, 2500-2560):
 * *out = (start, copies, period) triples in the reference's order (free with bwtmi_free) */
int bwtmi_index_lcp_plateaus(bwtmi_ctx *ctx, bwtmi_index *idx, const bwtmi_lib_params *p, int64_t **out,
                             int64_t *n);
/* find_short_imperfect_repeats(chromosome, tier1_seen) (bwt.py:2027-2095, 2562-2825): the
 * records are appended to job's final records with contig contig_id, whose sequence must be
 * the index text; seen = nseen (start, end) pairs (tier1_seen) */
int bwtmi_index_short_imperfect(bwtmi_ctx *ctx, bwtmi_index *idx, const bwtmi_lib_params *p,
                                const int64_t *seen, int64_t nseen, bwtmi_job *job, int32_t contig_id);
/* find_long_repeats(chromosome, tier1_seen) -> _find_repeats_simple (bwt.py:2097-2106,
 * 2177-2498): adaptive period/position scan with majority-vote extension; records appended to
 * job's final records with contig contig_id (the reference's extra 30 s wall-clock stop,
 * bwt.py:2238-2257, is not reproduced; its 100,000-iteration cap is) */
int bwtmi_index_long_repeats(bwtmi_ctx *ctx, bwtmi_index *idx, const bwtmi_lib_params *p,
                             const int64_t *seen, int64_t nseen, bwtmi_job *job, int32_t contig_id);
/* Tier1STRFinder(text_arr, max_motif_length).find_strs (bwt.py:1426-1538) over the full
 * sequence of the job's contig contig_id; records appended to the job's final records */
int bwtmi_job_tier1(bwtmi_ctx *ctx, bwtmi_job *job, int32_t contig_id, int32_t max_motif_length);
/* Tier3LongReadFinder(bwt_core).find_very_long_repeats(long_reads, chromosome) (bwt.py:2837-3036)
 * over the index (built over seq + '$'): reads = the reads' bytes back to back, read_off[nreads + 1]
 * their offsets (read_off[0] = 0).  The consolidated records get contig contig_id and go
 *   as_input = 0: to the job's final records (the library call's return value);
 *   as_input = 1: to the job's Tier 3 input of that contig, which bwtmi_job_postprocess joins after
 *                 the contig's strict hits before nested suppression (find_tandem_repeats_parallel,
 *                 bwt.py:3917-3924); call after bwtmi_job_reset and before bwtmi_job_scan. */
int bwtmi_index_tier3(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *reads, const int64_t *read_off,
                      int64_t nreads, bwtmi_job *job, int32_t contig_id, int32_t as_input);
/* BWTCore.backward_search (bwt.py:359-389) for npat patterns packed in pats,
 * pattern p = pats[off[p] .. off[p+1]).  Writes sp_ep[2p], sp_ep[2p+1]
 * (inclusive interval, or -1,-1). */
int bwtmi_backward_search_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *pats,
                                const int64_t *off, int64_t npat, int64_t *sp_ep);
/* Batched locate with substitutions on one or both strands (not in the
 * reference: BWTCore.locate_positions, bwt.py:398-410, is the exact,
 * one-pattern case).  T = the index text (n bytes, sentinel included),
 * pattern p = pats[off[p] .. off[p+1]), k = max_mismatch in 0..3.
 *   hit      (pos, strand, d) of a pattern P of m bytes: 0 <= pos, pos + m <= n,
 *            Q = P on strand '+' (0), revcomp(P) on strand '-' (1),
 *            d = |{ i : T[pos+i] != Q[i] }| <= k.  The comparison is bytewise
 *            as in backward_search: no case folding, 'N' is an ordinary byte.
 *   '$'      is never substituted: a window with a mismatching i where
 *            T[pos+i] == '$' is no hit (a '$' in the pattern still matches it
 *            exactly).  So k = 0 yields exactly the sorted SA[sp..ep] of
 *            backward_search, and no hit hangs over the end of a contig.
 *   revcomp  MotifUtils.reverse_complement (bwt.py:688) on bytes: A<->T, C<->G, every other
 *            byte unchanged, reversed.  '-' is searched only with
 *            BWTMI_LOCATE_BOTH_STRANDS and only when revcomp(P) != P (its hits
 *            would repeat the '+' ones).
 *   order    patterns in batch order; a pattern's hits by (pos, strand), '+'
 *            first; each (pattern, pos, strand) once.  hit_off[npat + 1] are the
 *            patterns' offsets into pos / mm (= d) / strand; *nhits = hit_off[npat].
 *   errors   BWTMI_E_ARG, never a silent empty result: an empty pattern,
 *            m < k + 1, m > 1024, k outside 0..3.  A pattern longer than the
 *            text, or (k = 0) with bytes the text lacks, is legal: no hits.
 *   cap      Q is split into k + 1 pieces, piece j = Q[floor(j m / (k+1)),
 *            floor((j+1) m / (k+1))).  The call's candidate count is the sum,
 *            over (pattern, searched strand, piece), of the piece's exact
 *            occurrences in T.  Above max_candidates (<= 0: the default 2^27,
 *            ~24 bytes of device scratch each) the call fails with
 *            BWTMI_E_NOMEM and the count in the message; nothing is truncated.
 *            *candidates (may be NULL) receives the count either way.
 * The four arrays are malloc'd (never NULL on success; free with bwtmi_free). */
#define BWTMI_LOCATE_BOTH_STRANDS 1u
int bwtmi_index_locate_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *pats, const int64_t *off,
                             int64_t npat, int32_t max_mismatch, uint32_t flags, int64_t max_candidates,
                             int64_t **hit_off, int64_t **pos, uint8_t **mm, uint8_t **strand, int64_t *nhits,
                             int64_t *candidates);
/* Batched SMEM seeding: the super-maximal exact matches of every query against
 * the index text, on one or both strands, with where they occur (not in the
 * reference).  T = the index text (n bytes, sentinel included), query q is
 * Q = qs[off[q] .. off[q+1]) of m bytes, 1 <= m <= 1024.  "Occurs" is plain
 * substring equality in T, bytes compared as backward_search compares them: no
 * case folding, 'N' and '$' are ordinary bytes, a byte absent from T occurs
 * nowhere.  No match wraps round the end of T: "$A" does not occur in "ACGT$"
 * (bwtmi_backward_search_batch, as the reference, reports that cyclic match).
 *   l(e)     matching statistics, e in 1..m: the largest l <= e such that
 *            Q[e-l, e) occurs in T; 0 when Q[e-1] does not occur.  Always
 *            l(e+1) <= l(e) + 1.
 *   SMEM     [s, e) with s = e - l(e) is an SMEM of Q when l(e) >= min_len and
 *            (e == m or l(e+1) <= l(e)); equivalently Q[s,e) occurs in T and
 *            neither Q[s-1,e) nor Q[s,e+1) does.  Within one strand the SMEMs
 *            of a query have strictly increasing s and e.
 *   strands  with BWTMI_SMEM_BOTH_STRANDS the same search runs on Q' =
 *            revcomp(Q) (the locate byte rule: A<->T, C<->G, every other byte
 *            unchanged, reversed).  An SMEM [s, e) of Q' is reported with strand
 *            1 and the coordinates of the original query, qstart = m - e, qend
 *            = m - s.  A query equal to its own reverse complement is searched
 *            on '+' only.
 *   count    the occurrences of the SMEM's string in T (the width of its SA
 *            interval).  count <= max_occ (<= 0: the default 1024): every
 *            occurrence start, ascending, in pos[pos_off[i] .. pos_off[i+1]);
 *            on strand 1 the forward-text start of the Q' match.  count >
 *            max_occ: the SMEM is still reported, with its count and an empty
 *            slice.
 *   cap      the call's position count is the sum of count over the SMEMs with
 *            count <= max_occ.  Above max_positions (<= 0: the default 2^27)
 *            the call fails with BWTMI_E_NOMEM and the count in the message;
 *            nothing is truncated.  *positions_total (may be NULL) receives the
 *            count either way.
 *   order    queries in batch order, smem_off[nq + 1] their offsets into the
 *            SMEM arrays; a query's SMEMs by (strand, qstart).
 *   work     *work (may be NULL) = the sum of l(e) over every searched string
 *            and every e: the rank steps the search is made of.
 *   errors   BWTMI_E_ARG: an empty query, m > 1024, min_len < 1, an unknown
 *            flag; every output pointer is then NULL and every count 0.  nq = 0
 *            is legal (smem_off = [0], pos_off = [0]), and so is min_len > m (no
 *            SMEMs).
 * One lane per end costs the sum of l(e) rank steps, m^2 / 2 for a read copied
 * from the text: hence the 1024-byte limit.  Longer reads go through
 * bwtmi_index_smem_long_batch below.
 * The seven arrays are malloc'd (never NULL on success; free with bwtmi_free):
 * smem_off[nq + 1]; qstart, qend, strand, count[*nsmem]; pos_off[*nsmem + 1];
 * pos[*npos]. */
#define BWTMI_SMEM_BOTH_STRANDS 1u
int bwtmi_index_smem_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                           int32_t min_len, uint32_t flags, int64_t max_occ, int64_t max_positions,
                           int64_t **smem_off, int32_t **qstart, int32_t **qend, uint8_t **strand, int64_t **count,
                           int64_t **pos_off, int64_t **pos, int64_t *nsmem, int64_t *npos,
                           int64_t *positions_total, int64_t *work);
/* The same search for long reads: the contract, arguments, outputs and errors
 * of bwtmi_index_smem_batch, word for word, with 1 <= m <= 1,048,576; for any
 * input that both entries accept the results are identical, `work` (still the
 * sum of l(e), exact) included.  The index must have been built with
 * BWTMI_INDEX_REVERSE, else BWTMI_E_STATE.  *steps (may be NULL) receives the
 * rank steps really taken, summed over the searched strings; on any error it is
 * 0 like the other counts (positions_total excepted, as above).
 *   how      one lane per searched string walks its SMEMs left to right: from
 *            a start i the match is extended rightwards to j = F(i) by plain
 *            backward steps in the reverse index; then l(e) = e - i for every
 *            end up to j, [i, j) is an SMEM (its SA interval comes from one
 *            backward search of Q[i, j) in the forward index, skipped when
 *            j - i < min_len), and the next start is s(j+1) = j + 1 - l(j+1),
 *            from one backward search from end j + 1 in the forward index.
 *   cost     about l(j+1) + 2 len rank steps per SMEM of len bytes: linear in m
 *            for a read that matches the text in a few long stretches (a whole
 *            3,000-byte text as its own query: 6,000 steps against work =
 *            4.5 M).  Worst case: SMEMs that overlap almost completely -- a
 *            read whose repeat tract is longer than the text's, "A" x 1600
 *            against "A" x 1500: 101 SMEMs of 1500 bytes, 450,000 steps on one
 *            lane -- are still m^2 / 2 and more, on a single lane. */
int bwtmi_index_smem_long_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                                int32_t min_len, uint32_t flags, int64_t max_occ, int64_t max_positions,
                                int64_t **smem_off, int32_t **qstart, int32_t **qend, uint8_t **strand,
                                int64_t **count, int64_t **pos_off, int64_t **pos, int64_t *nsmem, int64_t *npos,
                                int64_t *positions_total, int64_t *work, int64_t *steps);

/* ------------------------------------------------------------ chaining and read mapping
 * Colinear chaining of anchors (not in the reference): the step from a bag of
 * seeds to "where does this read lie, and how much longer or shorter is it
 * there than the text".
 *   anchor   (q, r, len), len >= 1: query bytes [q, q + len) equal text bytes
 *            [r, r + len).  qe = q + len, re = r + len.
 *   groups   anchors come in groups, group g = anchors [group_off[g],
 *            group_off[g + 1]); chaining never crosses a group.
 *   order    inside a group the anchors are ordered by (re, qe) ascending, ties
 *            in input order; the indices 0 .. A - 1 below are in this order.
 *   DP       all in integers:
 *              cost(d) = 0 if d == 0 else (d >> 4) + (bit_length(d) >> 1)
 *              f[i] = len_i; p[i] = -1
 *              for j = i - 1 down to max(0, i - max_pred):
 *                  dr = re_i - re_j;  if dr > max_gap: break
 *                  dq = qe_i - qe_j
 *                  if dq <= 0 or dr <= 0 or dq > max_gap: continue
 *                  d = |dr - dq|;     if d > bandwidth: continue
 *                  s = f[j] + min(len_i, dq, dr) - cost(d)
 *                  if s > f[i]: f[i], p[i] = s, j
 *            (strict: of predecessors with equal s the nearest, largest j, wins;
 *            the order is by re, so after the break nothing further qualifies).
 *   chains   per group: visit the anchors by (f descending, index ascending);
 *            skip a used anchor; otherwise walk i, p[i], p[p[i]], ... marking
 *            each anchor used, and stop at p = -1 or in front of an anchor u that
 *            is already used.  score = f[i] - (f[u] if the walk stopped at u else
 *            0).  The chain is kept when score >= min_score and it has at least
 *            min_anchors anchors; the marks stay either way.  A group's chains
 *            come out in visiting order.
 *   fields   of a chain: score, n_anchors, qstart = the minimum q of its
 *            anchors, qend = the maximum qe, rstart = the minimum r, rend = the
 *            maximum re, and its anchors in ascending index order.
 *   params   each field <= 0: the default -- max_gap 5000, bandwidth 500,
 *            max_pred 1024, min_score 40, min_anchors 1.  The defaults are
 *            choices (round numbers in the range read mappers use for reads of
 *            10^2..10^4 bytes), not measurements.  BWTMI_E_ARG before anything
 *            reaches the device: max_pred > 4096, bandwidth > max_gap (after
 *            the defaults), a nonzero reserved field.  params = NULL: all
 *            defaults. */
typedef struct {
    int32_t max_gap, bandwidth, max_pred, min_score, min_anchors, reserved[3];
} bwtmi_chain_params;
/* The device chainer (chain.hip) on a caller's anchors, exactly as
 * bwtmi_index_map_batch runs it (tests, embedders).
 *   in       group_off[ng + 1] (group_off[0] = 0), q / r / len[group_off[ng]].
 *   out      chain_off[ng + 1]: the groups' offsets into the chain arrays score,
 *            n_anchors, qstart, qend (int32), rstart, rend (int64), *nchain rows;
 *            member_off[*nchain + 1] into member[*nmember]: the input indices of
 *            each chain's anchors, in chain order.  All nine are malloc'd (never
 *            NULL on success; free with bwtmi_free).  *evals (may be NULL): the
 *            predecessors the DP evaluated, i.e. the j it reached before a break.
 *   errors   BWTMI_E_ARG with every output untouched: the parameter errors
 *            above, ng < 0, group_off[0] != 0 or decreasing offsets, len < 1,
 *            q < 0 or qe > 2^24, r < 0 or re > 2^32, a null anchor array with
 *            anchors present.  BWTMI_E_NOMEM: 2^31 anchors or groups and more.
 *            ng = 0 and empty groups are legal. */
int bwtmi_chain_anchors(bwtmi_ctx *ctx, const int64_t *group_off, int64_t ng, const int32_t *q, const int64_t *r,
                        const int32_t *len, const bwtmi_chain_params *params, int64_t **chain_off, int32_t **score,
                        int32_t **n_anchors, int32_t **qstart, int32_t **qend, int64_t **rstart, int64_t **rend,
                        int64_t **member_off, int64_t **member, int64_t *nchain, int64_t *nmember, int64_t *evals);
/* Batched read mapping: the SMEMs of every query (bwtmi_index_smem_batch's
 * arguments and search; with BWTMI_MAP_LONG bwtmi_index_smem_long_batch's, which
 * needs BWTMI_INDEX_REVERSE, else BWTMI_E_STATE, and lifts the 1024-byte limit
 * to 1,048,576), chained on the device.
 *   groups   one per searched string, that is (query, strand).
 *   anchors  one per listed position of every SMEM with count <= max_occ: for
 *            the SMEM [s, e) of the searched string (Q, or revcomp(Q) on strand
 *            1) at text position pos, (q, r, len) = (s, pos, e - s).  An SMEM
 *            above max_occ gives no anchors; *skipped_smems counts them.  The
 *            anchor count is the SMEM step's position count and max_positions
 *            caps it exactly as there (BWTMI_E_NOMEM, nothing truncated,
 *            *positions_total either way).
 *   out      chain_off[nq + 1]: the queries' offsets into strand (uint8), score,
 *            n_anchors, qstart, qend (int32), rstart, rend (int64); member_off
 *            [*nchain + 1] into the members' member_q, member_r, member_len.
 *            Query coordinates (qstart, qend, member_q) are the original
 *            query's on both strands, [m - e', m - s') for [s', e') of revcomp(Q):
 *            as SMEMs are reported, and PAF's convention.  A strand-1 chain's
 *            members still come in the chain's order, so their member_q descend.
 *   order    queries in batch order; a query's chains by strand, then in the
 *            chainer's visiting order.
 *   counts   (each may be NULL) *positions_total, *skipped_smems, *anchors,
 *            *evals (the DP's evaluated predecessors).
 *   errors   those of the SMEM entry chosen, the parameter errors above, an
 *            unknown flag; every output pointer is then NULL and every count 0
 *            (positions_total excepted, as above).
 * The twelve arrays are malloc'd (never NULL on success; free with bwtmi_free). */
#define BWTMI_MAP_LONG 4u
int bwtmi_index_map_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                          int32_t min_len, uint32_t flags, int64_t max_occ, int64_t max_positions,
                          const bwtmi_chain_params *params, int64_t **chain_off, uint8_t **strand, int32_t **score,
                          int32_t **n_anchors, int32_t **qstart, int32_t **qend, int64_t **rstart, int64_t **rend,
                          int64_t **member_off, int32_t **member_q, int64_t **member_r, int32_t **member_len,
                          int64_t *nchain, int64_t *nmember, int64_t *positions_total, int64_t *skipped_smems,
                          int64_t *anchors, int64_t *evals);

/* ------------------------------------------------------------ base-level alignment of chains
 * What the read looks like between a chain's anchors (not in the reference): a
 * banded edit-distance DP with traceback per inter-anchor gap on the device
 * (align.hip), stitched into one CIGAR per chain.  Everything is in integers
 * and in the searched string's coordinates: S = Q on strand 0, S = revcomp(Q)
 * on strand 1 (A<->T, C<->G, every other byte unchanged, reversed, as
 * everywhere else); T is the index text.
 *   segments a chain's anchors in chain order are (q_i, r_i, len_i), qe_i = q_i +
 *            len_i, re_i = r_i + len_i.  Block 0 is anchor 0 whole: len_0 columns
 *            of '='.  For i >= 1: dq = qe_i - qe_(i-1) and dr = re_i - re_(i-1),
 *            both > 0; t_i = min(len_i, dq, dr); gap i is a = S[qe_(i-1), qe_i -
 *            t_i) against b = T[re_(i-1), re_i - t_i), of m = dq - t_i and n = dr -
 *            t_i bytes; block i is t_i columns of '=' (the trimming of map.py's
 *            nmatch).  Blocks are taken on trust: their bytes are not compared.
 *   gap DP   delta = n - m, lo = min(0, delta) - W, hi = max(0, delta) + W.  A
 *            cell (i, j), 0 <= i <= m, 0 <= j <= n, is in the band when lo <= j -
 *            i <= hi.  D[0][0] = 0; any other in-band cell is the minimum of
 *              D[i-1][j-1] + (a[i-1] != b[j-1])
 *              D[i][j-1] + 1
 *              D[i-1][j] + 1
 *            over the candidates whose source cell exists and is in the band.
 *            Bytes compare by equality.
 *   trace    from (m, n); at each cell the first of these that reproduces
 *            D[i][j]: the diagonal ('=' when the bytes are equal, else 'X'), left
 *            ('D', one text byte), up ('I', one query byte).
 *   CIGAR    of a chain: blocks and gaps in order, adjacent equal operations
 *            merged; each a uint32 len << 4 | op with BAM's codes I = 1, D = 2,
 *            '=' = 7, X = 8.  On strand 1 it stays in S's order (PAF's rule).
 *   fields   per chain: nm = the bases in X, I and D; n_eq = the bases in '=';
 *            cols = all columns; the aligned span [q_0, qe_last) x [r_0,
 *            re_last): aq_start, aq_end in the original query's coordinates on
 *            both strands (as qstart / qend are), ar_start, ar_end.  The span
 *            can differ from the chain's rstart / rend, which are minima and
 *            maxima over the anchors.
 *   params   band = W: negative, the default 32; 0 is legal; above 1024,
 *            BWTMI_E_ARG.  max_cells <= 0: the default 2^30.  Both defaults are
 *            choices (a band that holds the indels of a read's gap next to a
 *            tract difference already counted in delta; a cap of 1 GiB of
 *            scratch), not measurements.  params = NULL: all defaults.
 *   cap      cells(gap) = (m + 1) (|delta| + 2 W + 1) when m > 0 and n > 0, else
 *            0; the call's count is the sum over its gaps.  Above max_cells the
 *            call fails with BWTMI_E_NOMEM and the count in the message; nothing
 *            is truncated.  *cells_total (may be NULL) receives the count either
 *            way.  The device's scratch for the DP is one byte per cell of the
 *            gaps that take a wave and at most 289 bytes per gap that takes a
 *            lane (the classes are under `out`).
 *   in       exactly the arrays bwtmi_index_map_batch returns (the two calls
 *            compose without conversion; hand-made chains can be fed in):
 *            chain_off[nq + 1] the queries' offsets into the chains, strand
 *            [nchain], member_off[nchain + 1] into member_q, member_r, member_len
 *            [nmember].  member_q is in the original query's coordinates; a
 *            strand-1 chain's members come in chain order.
 *   out      cigar_off[nchain + 1] (int64) into cigar[*ncigar] (uint32); nm, n_eq,
 *            cols, aq_start, aq_end (int32), ar_start, ar_end (int64), one per
 *            chain.  All nine are malloc'd (never NULL on success, nchain = 0
 *            included; free with bwtmi_free).  gaps (may be NULL) receives three
 *            counts: the gaps with m = 0, n = 0 or m = n = 1, which need no DP;
 *            the other gaps with both sides <= 16, one lane each; the rest, one
 *            wave each.
 *   errors   BWTMI_E_ARG before anything reaches the device, every output pointer
 *            NULL and every count 0: offsets that decrease or do not start at 0
 *            and end at nchain / nmember; strand > 1; a chain without a member;
 *            len < 1; a member outside its query, or r < 0, or re > the text's
 *            n; dq <= 0 or dr <= 0 between consecutive members; a gap side above
 *            65,535; a query of 2^28 bytes or more or a reference span of 2^30
 *            or more (an operation's length has 28 bits, cols 31); band > 1024;
 *            a nonzero reserved field.  nq = 0 and nchain = 0 are legal. */
typedef struct {
    int32_t band, reserved[3];
    int64_t max_cells;
} bwtmi_align_params;
int bwtmi_index_align_chains(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                             const int64_t *chain_off, const uint8_t *strand, const int64_t *member_off,
                             const int32_t *member_q, const int64_t *member_r, const int32_t *member_len,
                             int64_t nchain, int64_t nmember, const bwtmi_align_params *params, int64_t **cigar_off,
                             uint32_t **cigar, int32_t **nm, int32_t **n_eq, int32_t **cols, int32_t **aq_start,
                             int32_t **aq_end, int64_t **ar_start, int64_t **ar_end, int64_t *ncigar,
                             int64_t *cells_total, int64_t *gaps);

/* ------------------------------------------------------------ extension past the outer anchors
 * bwtmi_index_align_chains and, per chain, a scored banded DP with X-drop from
 * each outer anchor towards the read's end (align.hip): the alignment then ends
 * where the read ends, or where the match ends.  Inputs, S, T, blocks, gaps, the
 * gap DP and its band W are exactly those of bwtmi_index_align_chains (the
 * "middle" below is its CIGAR).  With |S| the query's bytes and tn the text's:
 *   tail     a = S[qe_last, |S|), of m bytes, against b = T[re_last, re_last +
 *            n), n = min(tn - re_last, m + We).  Cell (i, j), 0 <= i <= m, 0 <= j
 *            <= n, exists when |j - i| <= We.  H[0][j] = -G j.  For i >= 1, H[i][j]
 *            is the maximum over the sources that exist of
 *              H[i-1][j-1] + (a[i-1] == b[j-1] ? A : -B)
 *              H[i][j-1] - G
 *              H[i-1][j] - G
 *            Bytes compare by equality.  No zero floor, no per-cell pruning.
 *   rows     are computed in order i = 1, 2, ...; a row with no cell ends the
 *            extension.  The best cell starts as (0, 0) with score 0; a cell
 *            replaces it only when strictly greater, rows ascending, then j
 *            ascending: ties keep the smaller i, then the smaller j.  After row
 *            i, if best - max(row i) > X the extension ends: later rows do not
 *            exist (X-drop).
 *   trace    from the best cell to (0, 0); at each cell the first of diagonal
 *            ('=' or 'X'), left ('D') and up ('I') whose source exists and
 *            reproduces H[i][j]: the gap DP's preference.
 *   head     the same rule on the reversed strings: a'[i] = S[q_0 - 1 - i], m =
 *            q_0; b'[j] = T[r_0 - 1 - j], n = min(r_0, m + We); its operations
 *            are then reversed.
 *   empty    m = 0 or n = 0: no extension, score 0, no rows, no cells.
 *   result   the CIGAR is head, middle, tail, adjacent equal operations merged.
 *            nm, n_eq, cols and the span aq_* / ar_* include both extensions (the
 *            best cells' i lengthen the query span, their j the text span); aq_*
 *            stay in the original query's coordinates on both strands.
 *            head_score, tail_score (int32 per chain): the two best scores.
 *            *ext_rows (may be NULL): the rows computed, summed over all heads
 *            and tails of the call.
 *   params   band, max_cells: as bwtmi_align_params.  ext_band = We, default 32,
 *            0..1024; match = A, default 1, 1..64; mismatch = B, default 3, 0..64;
 *            gap = G, default 3, 1..64; xdrop = X, default 30, 0..2^20.  A negative
 *            value selects the default.  The defaults are choices (the penalties
 *            of a short-read aligner with a linear gap; an X that ten mismatches
 *            in a row exhaust), not measurements.  params = NULL: all defaults.
 *   cap      the call's count is the gaps' cells plus, per non-empty extension,
 *            (i* + 1) (2 We + 1) with i* the best cell's row.  The gaps' part is
 *            checked before anything reaches the device; the whole once the best
 *            cells are known.  Either way the call fails with BWTMI_E_NOMEM and
 *            the count in the message and in *cells_total; nothing is
 *            truncated.  The device's scratch for the extensions' directions is
 *            one byte per cell counted here, and two rows of 2 We + 2 ints per
 *            extension in flight.
 *   out      the nine arrays of bwtmi_index_align_chains, then head_score and
 *            tail_score: eleven malloc'd arrays (never NULL on success; free with
 *            bwtmi_free).  gaps as there: extensions are not gaps.
 *   errors   those of bwtmi_index_align_chains, a new field out of range, a
 *            nonzero reserved field, and a query with a chain of match * |Q| >=
 *            2^30 (a score has 31 bits): BWTMI_E_ARG before anything reaches the
 *            device, every output pointer NULL and every count 0. */
typedef struct {
    int32_t band, ext_band, match, mismatch, gap, xdrop, reserved[2];
    int64_t max_cells;
} bwtmi_extend_params;
int bwtmi_index_align_extend(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                             const int64_t *chain_off, const uint8_t *strand, const int64_t *member_off,
                             const int32_t *member_q, const int64_t *member_r, const int32_t *member_len,
                             int64_t nchain, int64_t nmember, const bwtmi_extend_params *params, int64_t **cigar_off,
                             uint32_t **cigar, int32_t **nm, int32_t **n_eq, int32_t **cols, int32_t **aq_start,
                             int32_t **aq_end, int64_t **ar_start, int64_t **ar_end, int32_t **head_score,
                             int32_t **tail_score, int64_t *ncigar, int64_t *cells_total, int64_t *gaps,
                             int64_t *ext_rows);

/* ------------------------------------------------------------ selection of a read's chains
 * Which of a read's chains is its placement, which are echoes of it, and how far
 * the placement is to be trusted (not in the reference): primary / secondary,
 * MAPQ and the pruning of weak secondaries, on the device (select.hip), before
 * any alignment.  The entry works on chain rows only and takes no index, so a
 * group may hold one read's chains from both strands and from several contigs'
 * indexes.  Everything is in integers, with products in 64 bits.
 *   in       chain_off[ng + 1] (chain_off[0] = 0): group g = chains [chain_off[g],
 *            chain_off[g + 1]); score, qstart, qend (int32), one per chain.  A
 *            group is one read.  qstart / qend are the original query's
 *            coordinates, as bwtmi_index_map_batch returns them, so intervals of
 *            both strands compare directly.
 *   rank     inside a group: by (score descending, input index ascending).
 *   parent   visit the group's chains in rank order, keeping the list P of
 *            primaries in the order found.  For chain c take the first p in P with
 *              ov(c, p) * 100 >= mask * min(qend_c - qstart_c, qend_p - qstart_p)
 *              ov = max(0, min(qend_c, qend_p) - max(qstart_c, qstart_p)).
 *            If there is one, c is secondary and parent[c] = p; if sub[p] is
 *            still 0, sub[p] = score_c (the best secondary, by the rank order).
 *            Otherwise c is primary: parent[c] = c, sub[c] = 0, and c is appended
 *            to P.  Overlap is judged per primary, never summed over primaries.
 *   keep     primaries: always.  Secondaries in rank order: c is kept when
 *              score_c * 100 >= pri_ratio * score_parent(c)
 *            and fewer than best_n secondaries of this group have been kept so far.
 *   mapq     primary: floor(60 * (s1 - sub) * min(s1, full) / (s1 * full)) with s1
 *            its score, in 0..60; secondary: 0.
 *   out      parent (int32: the parent's index relative to its group's first
 *            chain, in input order; a primary's own), sub (int32; 0 for a
 *            secondary and for a primary without one), mapq (uint8), keep (uint8
 *            0 / 1), one per chain in input order.  All four are malloc'd (never
 *            NULL on success, no chains included; free with bwtmi_free).
 *            *n_primary, *n_kept (each may be NULL): the primaries, and the kept
 *            chains, primaries included.
 *   params   a negative value selects the default: mask 50 (legal 1..100),
 *            pri_ratio 80 (0..100), best_n 5 (>= 0; 0 = primaries only), full 100
 *            (1..2^20).  The defaults are choices (the usual read-mapper values
 *            for the first three; a score at which a unique chain earns the full
 *            60), not measurements.  params = NULL: all defaults.
 *   errors   BWTMI_E_ARG before anything reaches the device, every output pointer
 *            NULL and every count 0: ng < 0; offsets that decrease or do not
 *            start at 0; qstart < 0, qend <= qstart or qend > 2^28; score < 1 or
 *            score > 2^30; mask 0 or > 100; pri_ratio > 100; full 0 or > 2^20; a
 *            nonzero reserved field; a null array with chains present.
 *            BWTMI_E_NOMEM: 2^31 chains or groups and more.  ng = 0 and empty
 *            groups are legal.  There is no cap on a group's size. */
typedef struct {
    int32_t mask, pri_ratio, best_n, full, reserved[4];
} bwtmi_select_params;
int bwtmi_select_chains(bwtmi_ctx *ctx, const int64_t *chain_off, int64_t ng, const int32_t *score,
                        const int32_t *qstart, const int32_t *qend, const bwtmi_select_params *params,
                        int32_t **parent, int32_t **sub, uint8_t **mapq, uint8_t **keep, int64_t *n_primary,
                        int64_t *n_kept);

/* ------------------------------------------------------------ repeat job
 * Replaces the per-contig worker result handling and the post-processing of
 * TandemRepeatFinder (bwt.py:3040-3141, 3402-3944) and save_results with
 * compound detection and the five writers (bwt.py:454-641, 3995-4198). */
typedef struct {
    int32_t min_copies;     /* --min-copies (default 3) */
    int32_t max_unit_len;   /* --max-unit-len (default 120) */
    int32_t show_progress;  /* --progress: lifts the >50 Mbp Tier-2 gate (bwt.py:3070) */
    int32_t tier2;          /* 0 when --tier1 (bwt.py:4257-4259) */
    int32_t threads;        /* host threads for post-processing (0 = auto) */
    int32_t build_index;    /* also build the FM index per contig in bwtmi_job_scan, as the
                               reference worker does (bwt.py:3053-3054); 0 = skip */
    int32_t sa_sample;      /* --sa-sample (default 32) */
    int32_t reserved;
} bwtmi_params;

#define BWTMI_FMT_STRFINDER 0
#define BWTMI_FMT_BED 1
#define BWTMI_FMT_VCF 2
#define BWTMI_FMT_TRF_TABLE 3
#define BWTMI_FMT_TRF_DAT 4

int bwtmi_job_create(const bwtmi_params *params, bwtmi_job **out);
int bwtmi_job_free(bwtmi_job *job);
/* register a contig: name, the full (untrimmed, upper-cased) sequence and the
 * trim offset; the analysed sequence is full[trim : full_len - trim_right]. */
int bwtmi_job_add_contig(bwtmi_job *job, const char *name, const uint8_t *full, int64_t full_len,
                         int64_t trim_left, int64_t trim_right, int32_t *contig_id);
/* run the worker on every registered contig on ctx's device (strict scan,
 * gates, Rule-1 filter) -- equivalent to find_tandem_repeats(_parallel) up to
 * all_repeats (bwt.py:3792-3822, 3850-3915) */
int bwtmi_job_scan(bwtmi_ctx *ctx, bwtmi_job *job);
/* the FM index builds of bwtmi_job_scan (build_index) run on the device behind
 * the host post-processing; this joins them (every other call on ctx, and
 * bwtmi_job_free, joins them too) and returns their error, if any */
int bwtmi_job_wait(bwtmi_ctx *ctx, bwtmi_job *job);
/* copy every contig to device memory now (bwtmi_job_scan does it on first use);
 * later scans reuse the resident copies */
int bwtmi_job_upload(bwtmi_ctx *ctx, bwtmi_job *job);
/* drop raw / final records so the job can be scanned again */
int bwtmi_job_reset(bwtmi_job *job);
int bwtmi_job_set_params(bwtmi_job *job, const bwtmi_params *params);
/* restrict bwtmi_job_scan to the listed contigs (this rank's shard); n < 0 = all */
int bwtmi_job_select(bwtmi_job *job, const int32_t *ids, int32_t n);
/* alternatively feed raw hits computed elsewhere (one contig at a time) */
int bwtmi_job_add_hits(bwtmi_job *job, int32_t contig_id, const bwtmi_hit *hits, int64_t n);
int64_t bwtmi_job_raw_count(const bwtmi_job *job);
/* nested suppression .. final filter (bwt.py:3926-3944) */
int bwtmi_job_postprocess(bwtmi_job *job);
int64_t bwtmi_job_count(const bwtmi_job *job);
/* render a format into a malloc'd buffer (free with bwtmi_free) or a file */
int bwtmi_job_render(bwtmi_job *job, int fmt, char **out, int64_t *len);
int bwtmi_job_write(bwtmi_job *job, int fmt, const char *path);
/* bwtmi_job_write returning once every row is formatted: the job's writer
 * thread finishes the file behind the caller (the header and each run of
 * formatted rows are written as they complete, in file order).
 * bwtmi_job_write_join waits for it and returns its error (BWTMI_E_IO: the file
 * is cut to 0 bytes); the job's next write or write_async, and bwtmi_job_free,
 * join it first (free drops the error).  Not in the reference: a caller that
 * writes one file per job (bwt.py:4141-4198) can overlap the file's tail with
 * its next job's load and scan. */
int bwtmi_job_write_async(bwtmi_job *job, int fmt, const char *path);
int bwtmi_job_write_join(bwtmi_job *job);
/* Sharded output (one process per GPU, each owning whole fold units = contigs
 * with equal natural sort keys, bwt.py:22-36): the file is the concatenation,
 * in unit order, of every unit's rows (bwt.py:4147-4150), so each rank writes
 * its own units at offsets from an exchange of sizes -- no record gather.
 *   unit_count              number of fold units (same on every rank)
 *   unit_rows[u]            local final records of unit u (VCF row ids)
 *   render_units            format the local units; bytes[0] = header size,
 *                           bytes[1 + u] = size of unit u (0 if not local);
 *                           row_base[u] = global VCF id of unit u's first row
 *                           (NULL: local numbering)
 *   write_units             pwrite the rendered units into `path` (opened
 *                           without truncation) at offsets[1 + u]; the header
 *                           at offsets[0] when write_header */
int32_t bwtmi_job_unit_count(bwtmi_job *job);
int bwtmi_job_unit_rows(bwtmi_job *job, int64_t *unit_rows);
int bwtmi_job_render_units(bwtmi_job *job, int fmt, const int64_t *row_base, int64_t *bytes);
int bwtmi_job_write_units(bwtmi_job *job, const char *path, const int64_t *offsets, int write_header);
/* the same behind the caller (the job's thread pwrites the rendered units);
 * bwtmi_job_write_join waits for it and returns its error */
int bwtmi_job_write_units_async(bwtmi_job *job, const char *path, const int64_t *offsets, int write_header);
/* final records (built on first use, see bwtmi_job_stage_ms; any thread) as
 * rows of int64: start, end, length, tier, n_copies_eval,
 * max_mm, score, flags (1: composition None / entropy 0.0, 2: k-mer scan piece),
 * chrom_id and doubles: copies, mismatch_rate, confidence, percent_matches,
 * percent_indels (for tests / the Python record view) */
int bwtmi_job_get_records(bwtmi_job *job, int64_t *ints9, double *dbls5);
/* strings of record i: which = 0 motif, 1 consensus, 2 variations(';'-joined),
 * 3 actual_sequence, 4 strand; returns length, copies up to cap bytes */
int64_t bwtmi_job_get_string(bwtmi_job *job, int64_t i, int which, char *buf, int64_t cap);
/* string `which` of every record, concatenated: offsets[0..count] (count + 1
 * entries, when offsets != NULL) and the bytes into buf when buf != NULL and
 * cap >= the total; returns the total byte count (-1: bad argument).  One
 * call per column for the Python record view instead of one per record. */
int64_t bwtmi_job_get_strings(bwtmi_job *job, int which, char *buf, int64_t cap, int64_t *offsets);
/* serialise final records for a gather to another rank; import appends them */
int bwtmi_job_export(bwtmi_job *job, uint8_t **buf, int64_t *len);
int bwtmi_job_import(bwtmi_job *job, const uint8_t *buf, int64_t len);
/* replace the final records by a serialised list (bwtmi_job_export's format;
 * save_results over a caller-built list of records, bwt.py:4141-4198);
 * bwtmi_wire_record_size = size of one fixed record header in that format */
int bwtmi_job_set_records(bwtmi_job *job, const uint8_t *buf, int64_t len);
int bwtmi_wire_record_size(void);
/* the worker's error of contig id in the last bwtmi_job_scan (0 = none): a
 * failing contig yields no records and the others go on, as the reference's
 * `except Exception: print("ERROR processing chromosome ..."); return []`
 * (bwt.py:3137-3141); copies the message, returns its length */
int64_t bwtmi_job_contig_error(const bwtmi_job *job, int32_t id, char *buf, int64_t cap);
/* per-stage wall times (ms) of the last scan/postprocess/render calls.  The
 * post-processing fills slots 2..5: screen+sort, dedup, merge, refine..filter.
 * Every fold unit runs merge, refine, collapse and the final filter in one
 * pass (over the segments between verified cuts; a unit of several contigs, a
 * contig with Tier 3 records, or any unit under BWTMI_FOLD_CUTS=0 is one
 * segment): `merge` is that pass with its cut bits, the gathering of its
 * survivors included; `refine..filter` is the time spent building records from
 * them inside postprocess -- 0 when every unit with records is one contig:
 * the job then keeps the survivors, the writers read those, and records are
 * built by the first call that asks for them (bwtmi_job_get_records,
 * _get_string(s), _export; before _import, _set_records, the Tier entry
 * points, a new contig or load). */
int bwtmi_job_stage_ms(const bwtmi_job *job, double *out8);

/* Shard layout over ranks (replaces the Pool over contigs, bwt.py:3850-3912):
 * fold units (contigs with equal natural sort keys, bwt.py:22-36) go to ranks
 * by longest-processing-time greedy over their analysed lengths (ties: lower
 * unit, then lower rank).  Restricts the job to rank's contigs; ids (may be
 * NULL, else room for every contig) receives them ascending, n their count. */
int bwtmi_job_select_shard(bwtmi_job *job, int32_t world, int32_t rank, int32_t *ids, int32_t *n);

/* host CPUs this process may use (affinity mask, cgroup quota), the ranks on
 * this node (LOCAL_WORLD_SIZE) and the post-processing threads per rank that
 * follow from them (threads = 0 in bwtmi_params) */
int bwtmi_host_info(int32_t *cpus_visible, int32_t *local_world, int32_t *threads);

/* ------------------------------------------------------------ collective
 * The multi-GPU path's only exchange: RCCL (over xGMI) all-reduce of small
 * host vectors -- per-unit row / byte counts for the sharded output file and
 * the step time.  librccl is loaded on first use.  The 128-byte id comes from
 * bwtmi_comm_unique_id on one rank and reaches the others out of band
 * (bwtmi/comm.py: a TCP rendezvous next to MASTER_ADDR:MASTER_PORT). */
typedef struct bwtmi_comm bwtmi_comm;
int bwtmi_comm_unique_id(uint8_t *id /* 128 bytes */);
int bwtmi_comm_init(int32_t device, int32_t world, int32_t rank, const uint8_t *id, bwtmi_comm **out);
/* in place over `count` host values; dtype 0 = int64, 1 = float64; op 0 = sum, 1 = max */
int bwtmi_comm_allreduce(bwtmi_comm *comm, void *vals, int64_t count, int32_t dtype, int32_t op);
int bwtmi_comm_free(bwtmi_comm *comm);
/* hipDeviceSynchronize on device (bench step brackets) */
int bwtmi_device_sync(int32_t device);

/* ------------------------------------------------------------ helpers
 * MotifUtils.align_repeat_region (bwt.py:998-1102) -- the banded per-copy
 * alignment used by merge/refine; exposed for the Python MotifUtils mirror.
 * max_indel < 0 means None.  Returns 1 with a summary, 0 for None.
 * ints8: copies, motif_len, consumed, max_errors, tot_ins, tot_del, 0, 0;
 * mismatch_rate; consensus (motif_len bytes) and variations (';'-joined,
 * malloc'd, free with bwtmi_free); copy_len/copy_err (malloc'd int64[copies]). */
int bwtmi_align_region(const char *seq, int64_t seq_len, int64_t start, int64_t end, const char *tmpl,
                       int64_t tmpl_len, double frac, int64_t max_indel, int64_t min_copies,
                       int64_t *ints8, double *mismatch_rate, char *consensus, char **variations,
                       int64_t **copy_len, int64_t **copy_err);
/* ------------------------------------------------------------ FASTA
 * TandemRepeatFinder.load_reference (bwt.py:3713-3756) natively: strip,
 * '>' headers (name = first whitespace token), upper-case sequence lines,
 * blank lines skipped, duplicate names overwrite in place.  Registers every
 * contig in job (trim = flank_trim if len > 2*flank_trim). */
int bwtmi_job_load_fasta(bwtmi_job *job, const char *path, int32_t flank_trim);
/* bwtmi_job_load_fasta + bwtmi_job_upload for a whole file, with the analysed
 * sequences built on ctx's device from the file image: its copy to the device
 * overlaps the loader's first pass, the plain chunks (whole lines of
 * 0x21..0x7f bytes other than '>') are rebuilt there (fasta_dev.hip), and the
 * host copies of those chunks are written behind the device work -- complete
 * when the next bwtmi_job_scan returns, or when any other call on the job
 * reads contig bytes (bwtmi_job_contig_seq, postprocess, render, ...).
 * Replaces the same load_reference (bwt.py:3713-3756) as bwtmi_job_load_fasta. */
int bwtmi_job_load_fasta_dev(bwtmi_ctx *ctx, bwtmi_job *job, const char *path, int32_t flank_trim);
/* the device copy of contig `id`'s analysed (trimmed) sequence into dst
 * (trimmed_len bytes); fails when it is not resident on ctx's device */
int bwtmi_job_device_text(bwtmi_ctx *ctx, bwtmi_job *job, int32_t id, uint8_t *dst);
/* the same for rank `rank` of `world` processes: every contig is registered
 * (names and analysed lengths, for the shard layout), but only the fold units
 * this rank owns (bwtmi_job_select_shard) get their bases, and the job is
 * restricted to them */
int bwtmi_job_load_fasta_shard(bwtmi_job *job, const char *path, int32_t flank_trim, int32_t world,
                               int32_t rank);
/* Split multi-rank load (no rank reads the whole file): rank r runs the
 * loader's first pass over its 1/world of the file and returns a part table
 * (int64 words, freed with bwtmi_free); the ranks exchange the tables (an
 * all-gather, bwtmi.comm); bwtmi_job_load_fasta_parts takes all of them in
 * rank order, builds the contig table (names, lengths, trims, fold units --
 * identical on every rank), restricts the job to this rank's shard and reads
 * only those contigs' bytes.  A non-ASCII byte anywhere fails every rank.
 * Replaces load_reference (bwt.py:3713-3756) + the contig split of 3850-3912. */
int bwtmi_job_fasta_scan_part(bwtmi_job *job, const char *path, int32_t world, int32_t rank, int64_t **blob,
                              int64_t *nwords);
/* the same, and the part's bytes go up to ctx's device at once: a following
 * bwtmi_job_load_fasta_parts_dev on that ctx whose contigs lie inside the part
 * skips their copy (it overlapped the part-table exchange) */
int bwtmi_job_fasta_scan_part_dev(bwtmi_ctx *ctx, bwtmi_job *job, const char *path, int32_t world, int32_t rank,
                                  int64_t **blob, int64_t *nwords);
/* header lines of a FASTA file ('>' at the start or after a line break),
 * counted up to limit; -1 if it cannot be read.  Host only (no device is
 * touched): the CLI's decision to launch one rank per GPU (bwt.py:3863-3864's
 * Pool size) before anything initialises a GPU */
int64_t bwtmi_fasta_count_records(const char *path, int64_t limit);
int bwtmi_job_load_fasta_parts(bwtmi_job *job, const char *path, int32_t flank_trim, int32_t world, int32_t rank,
                               const int64_t *blob, int64_t nwords);
/* the same with this rank's analysed sequences built on ctx's device
 * (bwtmi_job_load_fasta_dev's placement: plain chunks rebuilt there from the
 * own contigs' bytes, host copies written behind the next scan) */
int bwtmi_job_load_fasta_parts_dev(bwtmi_ctx *ctx, bwtmi_job *job, const char *path, int32_t flank_trim,
                                   int32_t world, int32_t rank, const int64_t *blob, int64_t nwords);
int32_t bwtmi_job_contig_count(const bwtmi_job *job);
/* analysed length of contig id (its shard weight), also for contigs whose bases
 * live on another rank */
int64_t bwtmi_job_contig_weight(const bwtmi_job *job, int32_t id);
int64_t bwtmi_job_contig_info(const bwtmi_job *job, int32_t id, char *name, int64_t cap,
                              int64_t *full_len, int64_t *trim_left, int64_t *trim_right);
int bwtmi_job_contig_seq(const bwtmi_job *job, int32_t id, uint8_t *dst /* full_len */);

#ifdef __cplusplus
}
#endif
#endif /* BWTMI_H */
