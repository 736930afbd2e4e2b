/*
 * fqz5_fastq.h — FASTQ text in device memory to fqzcomp5 blocks and back
 * (SURVEY §8 f3), on the GPU:
 *
 *   fqz5_fastq_index    load_seqs_kseq's record parse (fqzcomp5.c:423-623,
 *                       kseq.h:178-218) for 4-line FASTQ: name up to the
 *                       first isspace(), comment to the line end, one
 *                       sequence line, '+' line, one quality line, a
 *                       trailing '\r' dropped as kseq drops it.  Text whose
 *                       first byte is '>' is FASTA: a record per header
 *                       line, its sequence lines joined as kseq joins them
 *                       (kseq.h:194-198; no quality section in its blocks,
 *                       fqzcomp5.c:575-578, :2258-2264); a bare '>' as the
 *                       last line is no record.  Other text fails
 *                       (multi-line FASTQ); it is never parsed on the host.
 *   fqz5_fastq_blocks   the block split rule (fqzcomp5.c:471-479): a record
 *                       that would take a non-empty block past blk_size
 *                       (name.l + 1 + seq.l + qual.l per record) starts the
 *                       next block.
 *   fqz5_fastq_gather   one block's section inputs: names (name [' '
 *                       comment] '\0'), bases, qualities - 33 (device), the
 *                       record lengths and READ2 flags (host).
 *   fqz5_fastq_format(_pairs) output_fastq (fqzcomp5.c:3441-3480) of a decoded
 *                       block: '@' name '\n' seq '\n' '+' [name] '\n'
 *                       qual + 33 '\n'; without qualities output_fasta
 *                       (:3503-3517): '>' name '\n' seq '\n'.
 *   fqz5_fastq_format_range  the same text for a range of a block's records
 *                       only (record ranges read through the file's block
 *                       index, fqz5file.extract_file), laid out on the device.
 *   fqz5_fastq_format_list   the same for an ascending list of its records.
 *   fqz5_names_*        lookup by read name: a query table built on the host,
 *                       matched against a decoded name section on the device
 *                       (fqz5file.find_names / extract_names_file).
 *   fqz5_seqs_*         lookup by sequence content: a pattern table built on
 *                       the host, matched against a block's decoded bases.
 *   fqz5_stats_*        read QC statistics: a block's decoded bases and
 *                       qualities histogrammed into a device accumulator
 *                       (fqz5file.stats).
 *   fqz5_filter_*       filter by read metrics: the records of a block whose
 *                       length, N count, mean quality, low-quality share, GC
 *                       share and complexity pass a rule, picked on the
 *                       device (fqz5file.filter_records / filter_file).
 *   fqz5_trim_*         trim and clip: per record the interval of its bases
 *                       and qualities kept after the clip, quality, adapter,
 *                       N and crop steps, found on the device, and the
 *                       streams compacted to it (fqz5file.trim_records /
 *                       trim_file).
 *   fqz5_dedup_*        duplicates: per unit a 128-bit key of its bases summed
 *                       on the device, and a device table over the whole file
 *                       that keeps each key's first unit and count
 *                       (fqz5file.dedup_records / dedup_file / duplication).
 *
 * Offsets are bytes into the text.  Calls return 0 (fqz5_fastq_index: 1 for
 * FASTA text; fqz5_fastq_blocks: the block count) or -1 with
 * fqz5_last_error() set.
 */
#ifndef FQZ5_FASTQ_H
#define FQZ5_FASTQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {                  /* one record of the text */
    uint64_t name, comment, seq, qual;        /* offsets */
    uint32_t name_len, comment_len, seq_len;  /* kseq's name.l, comment.l, seq.l */
    uint32_t fasta;                           /* 1: FASTA, its sequence lines
                                                 in [seq, qual); 2: wrapped
                                                 FASTQ, sequence and quality
                                                 lines from seq and qual */
    uint64_t end;                             /* the offset after the record's
                                                 last line ('\n' included), never
                                                 above len; FASTA: the next
                                                 header's offset (a bare '>' that
                                                 ends the text included) or len */
} fqz5_fastq_rec;

/* Index the records of d_text[0..len) (device) into d_recs (device, max_rec
 * entries; len / 6 + 1 always suffice for 4-line FASTQ, the number of lines
 * for FASTA, whose shortest record is ">\n"); *nrec receives their number and
 * h_rec_size (host, max_rec entries, may be NULL) each record's
 * load_seqs_kseq size. */
int fqz5_fastq_index(const uint8_t *d_text, uint64_t len, fqz5_fastq_rec *d_recs,
                     uint64_t max_rec, uint64_t *nrec, uint32_t *h_rec_size);

/* fqz5_fastq_index for every layout kseq_read reads (kseq.h:178-218): 4-line
 * FASTQ, FASTA, and wrapped FASTQ (sequence and quality split over several
 * lines each; records with fasta = 2).  fqz5_fastq_index itself takes 4-line
 * FASTQ and FASTA only (the multi-GPU windows count records in lines). */
int fqz5_fastq_index_any(const uint8_t *d_text, uint64_t len, fqz5_fastq_rec *d_recs,
                         uint64_t max_rec, uint64_t *nrec, uint32_t *h_rec_size);

/* The ends (exclusive text offsets, increasing) of the complete FASTQ
 * records of d_text[0..len) (device; 4-line or wrapped): a record that the
 * text cuts off is left out unless eof (then the text end closes the last
 * one).  h_ends (host) holds up to max_ends; *n_ends receives the count.
 * Returns 0, or -1 on text that is not FASTQ kseq reads the same way. */
int fqz5_fastq_record_ends(const uint8_t *d_text, uint64_t len, int eof, uint64_t *h_ends,
                           uint64_t max_ends, uint64_t *n_ends);

/* Block starts (host): first[k] = the first record of block k, first[n] =
 * nrec.  Returns n, or -1 when more than max_blocks. */
int fqz5_fastq_blocks(const uint32_t *rec_size, uint64_t nrec, uint32_t blk_size,
                      uint64_t *first, int max_blocks);

/* Records [a, b) as one block.  sizes[3] receives the bytes of the names,
 * bases and qualities; with d_names / d_seq NULL only the sizes are
 * computed; d_qual NULL (FASTA): no qualities (sizes[2] = 0).  h_len / h_flag (host, b - a entries, may be NULL): record
 * lengths and FQZ5 READ2 flags (fqzcomp5.c:518-527). */
int fqz5_fastq_gather(const uint8_t *d_text, const fqz5_fastq_rec *d_recs, uint64_t a,
                      uint64_t b, uint8_t *d_names, uint8_t *d_seq, uint8_t *d_qual,
                      uint32_t *h_len, uint32_t *h_flag, uint64_t *sizes);

/* FASTQ text of a block (names '\0' after each, bases, qualities - 33 on
 * the device; lengths on the host) into d_out (out_cap bytes); *out_len its
 * size.  d_qual NULL: FASTA text.  d_out NULL: the size only. */
int fqz5_fastq_format(const uint8_t *d_names, uint64_t name_len, const uint8_t *d_seq,
                      const uint8_t *d_qual, const uint32_t *h_len, uint64_t nrec,
                      int plus_name, uint8_t *d_out, uint64_t out_cap, uint64_t *out_len);

/* Paired output (fqzcomp5 -d in out1 out2: output_fastq_deinterleaved /
 * output_fasta_deinterleaved, fqzcomp5.c:3535-3549, :3612-3676): as
 * fqz5_fastq_format, the block's even records (R1) first and its odd
 * records (R2) after them; *r1_len the first text's size. */
int fqz5_fastq_format_pairs(const uint8_t *d_names, uint64_t name_len, const uint8_t *d_seq,
                            const uint8_t *d_qual, const uint32_t *h_len, uint64_t nrec,
                            int plus_name, uint8_t *d_out, uint64_t out_cap, uint64_t *out_len,
                            uint64_t *r1_len);

/* The text of records [rec_first, rec_first + rec_count) of a block alone:
 * exactly the bytes fqz5_fastq_format (pairs != 0: fqz5_fastq_format_pairs,
 * the slice's even records of the block first, its odd ones after them;
 * *r1_len, may be NULL, the first part's size) writes for those records, the
 * slice's first record at d_out[0].  d_names, name_len, d_seq, d_qual, h_len
 * and nrec are the whole block's, as for fqz5_fastq_format (h_len is read up
 * to the slice end); the caller clips the slice: rec_first + rec_count > nrec
 * fails, as do fewer name terminators than rec_first + rec_count and a text
 * larger than out_cap.  rec_count 0: *out_len = 0, nothing is launched.
 * d_out NULL: the sizes only.  The layout (record sizes, output and sequence
 * offsets) is computed on the device by scans; only the totals come back. */
int fqz5_fastq_format_range(const uint8_t *d_names, uint64_t name_len, const uint8_t *d_seq,
                            const uint8_t *d_qual, const uint32_t *h_len, uint64_t nrec,
                            uint64_t rec_first, uint64_t rec_count, int plus_name, int pairs,
                            uint8_t *d_out, uint64_t out_cap, uint64_t *out_len,
                            uint64_t *r1_len);

/* fqz5_fastq_format_range for a list of records instead of a range: d_sel
 * (device, n_sel entries) holds record indices of the block, strictly
 * ascending and below nrec; the text is exactly the bytes fqz5_fastq_format
 * (pairs != 0: fqz5_fastq_format_pairs, the listed even records first, the
 * listed odd ones after them; *r1_len, may be NULL, the first part's size)
 * writes for those records, in that order.  h_len is read for all nrec
 * records.  The list is checked on the device: one that does not ascend or
 * reaches nrec fails the call, as do fewer name terminators than nrec and a
 * text larger than out_cap.  n_sel 0: *out_len = 0, nothing is launched.
 * d_out NULL: the sizes only.  The layout is computed on the device as for a
 * range (the sequence offsets a scan over all lengths, the output offsets a
 * scan over the listed records' sizes); only the totals come back. */
int fqz5_fastq_format_list(const uint8_t *d_names, uint64_t name_len, const uint8_t *d_seq,
                           const uint8_t *d_qual, const uint32_t *h_len, uint64_t nrec,
                           const uint32_t *d_sel, uint64_t n_sel, int plus_name, int pairs,
                           uint8_t *d_out, uint64_t out_cap, uint64_t *out_len, uint64_t *r1_len);

/* Lookup by read name (name_match.hip; fqz5file.find_names): a table of
 * query names built on the host, and the records of a decoded name section
 * (name [' ' comment] '\0' per record) whose key is one of them.  whole = 0:
 * a record's key is its name up to the first ' ' or '\t' (kseq's name);
 * whole != 0: the entire header line up to the '\0'.  Keys are compared byte
 * for byte; a mate suffix ("/1", "/2") is part of the key. */
typedef struct fqz5_name_table fqz5_name_table;

/* q: the queries, '\0' after each (the layout of a name section);
 * tag_bits 1..32: the file path passes 32, fewer only narrows the tag so that
 * tests reach the byte comparison.  An empty query and a query given twice
 * are refused (NULL). */
fqz5_name_table *fqz5_names_table_build(const uint8_t *q, uint64_t q_len, uint64_t nq,
                                        int tag_bits);

/* the table and its device copy (made by the first fqz5_names_match) */
void fqz5_names_table_free(fqz5_name_table *);

/* host probe with the kernel's hash and rule: query index or -1 */
int64_t fqz5_names_table_find(const fqz5_name_table *, const uint8_t *key, uint64_t len);

/* bytes of the kernel's LDS staging window */
uint32_t fqz5_names_match_window(void);

/* The records of d_names[0..name_len) (device; nrec records) whose key is in
 * the table: their indices, ascending, into d_rec and each one's query index
 * into d_query (device, nrec entries each), *n_hit their number.  pairs != 0:
 * a hit on record 2k or 2k + 1 selects both (a mate past nrec is ignored);
 * the query index of one that did not match itself is 0xFFFFFFFF.  Fails
 * when the section has fewer name terminators than nrec. */
int fqz5_names_match(const fqz5_name_table *, const uint8_t *d_names, uint64_t name_len,
                     uint64_t nrec, int whole, int pairs,
                     uint32_t *d_rec, uint32_t *d_query, uint64_t *n_hit);

/* Lookup by sequence content (seq_match.hip; fqz5file.find_seqs): a table of
 * patterns built on the host, and the records of a block's decoded bases
 * (the records' sequences one after the other, no separators) that contain
 * one of them as a contiguous substring.  Bytes are compared as they are
 * (case matters, 'N' is a byte like any other); an occurrence never spans two
 * records.  The table is keyed by the patterns' first m bytes, the anchor:
 * the hash and slot rule of the name table, but patterns may share an anchor
 * (separate slots of one probe, every tag match verified). */
typedef struct fqz5_seq_table fqz5_seq_table;

/* q: nq patterns, '\0' after each (as fqz5_names_table_build); tag_bits
 * 1..32 (the file path passes 32).  anchor: 0 = min(the shortest pattern,
 * 12), else the anchor length to use, at most 64 (tests force 1).  Refused
 * (NULL): no pattern, an empty one, a duplicate, more than 2^20 patterns, a
 * pattern longer than 65535 bytes, an anchor above the shortest pattern. */
fqz5_seq_table *fqz5_seqs_table_build(const uint8_t *q, uint64_t q_len, uint64_t nq,
                                      int tag_bits, int anchor);

/* the table and its device copy (made by the first fqz5_seqs_match) */
void fqz5_seqs_table_free(fqz5_seq_table *);

/* the anchor length in use */
uint32_t fqz5_seqs_table_anchor(const fqz5_seq_table *);

/* bases per workgroup tile of the kernel */
uint32_t fqz5_seqs_match_tile(void);

/* Host restatement of the kernel's rule, one thread, no GPU: hit[r] (nrec
 * entries) = the lowest pattern index occurring in record r, or 0xFFFFFFFF;
 * seen[q] |= 1 (nq bytes, may be NULL) where pattern q occurs in some record.
 * lens: the records' lengths; fails when they do not sum to seq_len. */
int fqz5_seqs_scan_host(const fqz5_seq_table *, const uint8_t *seq, uint64_t seq_len,
                        const uint32_t *lens, uint64_t nrec, uint32_t *hit, uint8_t *seen);

/* d_seq[0..seq_len) (device) holds the bases of nrec records whose lengths
 * are h_len (host).  The records that contain a pattern: their indices,
 * ascending, into d_rec and each one's lowest pattern index into d_query
 * (device, nrec entries each), *n_hit their number.  pairs != 0: a hit on
 * record 2k or 2k + 1 selects both (a mate past nrec is ignored); the query
 * index of one that did not match itself is 0xFFFFFFFF.  d_seen (device, nq
 * bytes, may be NULL): byte q is set to 1 where pattern q occurs in some
 * record, also where a lower pattern occurs in every such record; it is never
 * cleared, so one buffer serves a whole file.  Fails when the lengths do not
 * sum to seq_len or nrec >= 2^31. */
int fqz5_seqs_match(const fqz5_seq_table *, const uint8_t *d_seq, uint64_t seq_len,
                    const uint32_t *h_len, uint64_t nrec, int pairs,
                    uint32_t *d_rec, uint32_t *d_query, uint64_t *n_hit, uint8_t *d_seen);

/* Read QC statistics (stats.hip; fqz5file.stats): counts over the decoded
 * bases and qualities of a file's blocks, added block by block into one
 * device accumulator.  mates is 1 or 2; with 2, record r of a block belongs
 * to mate r & 1 and a block holds whole pairs.  A quality q is the quality
 * line's byte - 33 (what the decoder leaves on the device).
 *
 * The tables are u64 words, one mate's after the other; a mate's
 * W = 873 + 262 * cycles words are
 *     [0] records  [1] bases  [2] qual_records (records of blocks that have
 *     qualities)  [3] empty (records of length 0)
 *     [4, 260)     base_counts[256]  count of each sequence byte, case kept
 *     [260, 516)   qual_counts[256]  count of each q
 *     [516, 772)   read_qual[256]    records of length L > 0 with qualities,
 *                                    by floor(sum(q) / L)
 *     [772, 873)   read_gc[101]      records of length L > 0, by
 *                                    floor(100 * gc / L), gc its bytes in "GCgc"
 *     [873, 873 + 6 * cycles)        cycle_base[cycles][6]: at position c, the
 *                                    records longer than c by the class of
 *                                    their byte there: A, C, G, T, N, other
 *                                    (case folded)
 *     [873 + 6 * cycles, W)          cycle_qual[cycles][256]: likewise by q
 * Positions at or past `cycles` count in the whole-file tables only. */
typedef struct fqz5_stats fqz5_stats;

/* a zeroed accumulator on the calling thread's device; cycles 1..65536
 * (NULL with fqz5_last_error() set otherwise) */
fqz5_stats *fqz5_stats_new(uint32_t cycles, int mates);
void fqz5_stats_free(fqz5_stats *);

/* mates * W: the words fqz5_stats_read and fqz5_stats_host fill */
uint64_t fqz5_stats_words(uint32_t cycles, int mates);

/* bases per tile of the kernels */
uint32_t fqz5_stats_tile(void);

/* Add one block: d_seq[0..seq_len) and d_qual[0..seq_len) (device; d_qual
 * NULL: a block without qualities, the quality tables and qual_records stay
 * as they are) hold nrec records whose lengths are h_lens (host).  d_rec_qsum
 * / d_rec_gc (device, nrec entries each, either may be NULL): per record the
 * sum of its q (0 without qualities) and its number of G/C bytes, the values
 * read_qual and read_gc are binned from.  The record ends are uploaded once
 * per call.  Fails when the lengths do not sum to seq_len, on an odd nrec
 * with two mates, or nrec >= 2^31, each before anything is added. */
int fqz5_stats_add(fqz5_stats *, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t seq_len,
                   const uint32_t *h_lens, uint64_t nrec, uint64_t *d_rec_qsum,
                   uint32_t *d_rec_gc);

/* the tables so far into h_out (host, cap words, at least fqz5_stats_words) */
int fqz5_stats_read(const fqz5_stats *, uint64_t *h_out, uint64_t cap);

/* Host restatement of the kernels' rule, one thread, no GPU: the block's
 * counts are added to h_out (the same layout, cap words; zero it before the
 * first block); rec_qsum / rec_gc (host, may be NULL) as above.  Fails as
 * fqz5_stats_new and fqz5_stats_add do, before anything is added. */
int fqz5_stats_host(uint32_t cycles, int mates, const uint8_t *seq, const uint8_t *qual,
                    uint64_t seq_len, const uint32_t *lens, uint64_t nrec, uint64_t *h_out,
                    uint64_t cap, uint64_t *rec_qsum, uint32_t *rec_gc);

/* Filter by read metrics (filter.hip; fqz5file.filter_records): which records
 * of a block's decoded bases and qualities are worth keeping.  The rule is
 * exact integer arithmetic, every product in u64, and the device and
 * fqz5_filter_host agree bit for bit.  Per record:
 *     L     its length
 *     n     its bytes in "Nn"
 *     gc    its bytes in "GCgc"
 *     diff  the positions 0 <= i < L - 1 with s[i] != s[i + 1], bytes compared
 *           as they are; a neighbour in the next record never counts
 *     qsum  the sum of its q (the quality line's byte - 33, as the decoder
 *           leaves it)
 *     lowq  its q below low_q (0 unless criterion 4 is set)
 * A criterion counts only where its bit (1 << index) is in `set`:
 *     0 min_len             L >= min_len
 *     1 max_len             L <= max_len
 *     2 max_n               n <= max_n
 *     3 min_mean_q          qsum >= min_mean_q * L
 *     4 low_q, max_low_pct  100 * lowq <= max_low_pct * L
 *     5 gc_min_pct, gc_max_pct
 *                           gc_min_pct * L <= 100 * gc <= gc_max_pct * L
 *     6 min_complexity_pct  100 * diff >= min_complexity_pct * max(L - 1, 0)
 * so with L = 0 criteria 2..6 hold and the lengths alone decide.  A record
 * passes when it passes every criterion that is set; its reason is the lowest
 * index it fails.  A unit is one record, with pairs the records 2k and 2k + 1:
 * a pair passes only when both mates pass (the lookups take a pair on either
 * mate), and its reason is the lowest index either mate fails.  The selected
 * units are those that pass, with invert exactly those that do not. */
#define FQZ5_FILTER_REASONS 7
typedef struct {
    uint32_t set;                 /* bit k: criterion k counts */
    uint32_t min_mean_q, low_q, max_low_pct, gc_min_pct, gc_max_pct, min_complexity_pct;
    uint64_t min_len, max_len, max_n;
} fqz5_filter_spec;

/* per record (nrec entries each; any may be NULL): the sums above */
typedef struct {
    uint32_t *n, *gc, *diff;
    uint64_t *qsum;
    uint32_t *lowq;
} fqz5_filter_sums;

/* bases per tile of the sums kernel */
uint32_t fqz5_filter_tile(void);

/* d_seq[0..seq_len) and d_qual[0..seq_len) (device) hold nrec records whose
 * lengths are h_len (host).  The selected records' indices go, ascending,
 * into d_rec (device, nrec entries; both mates of a selected pair), *n_hit
 * their number; h_failed[reason] (host, 7 words, added to) counts the units
 * that failed, whether or not invert selects them.  The bases are streamed
 * only when one of criteria 2, 5, 6 is set or d_sums is given, the qualities
 * only when 3 or 4 is set or d_sums is given; a stream that is not needed may
 * be NULL (both with length criteria alone: no sums kernel runs), and one that
 * is NULL leaves its sums 0.  d_sums (may be NULL): device arrays that
 * receive the per-record sums.  Fails, before anything is written: criterion
 * 2, 5 or 6 with d_seq NULL, criterion 3 or 4 with d_qual NULL, lengths that
 * do not sum to seq_len, nrec >= 2^31, an odd nrec with pairs. */
int fqz5_filter_match(const fqz5_filter_spec *, const uint8_t *d_seq, const uint8_t *d_qual,
                      uint64_t seq_len, const uint32_t *h_len, uint64_t nrec, int pairs,
                      int invert, uint32_t *d_rec, uint64_t *n_hit, uint64_t *h_failed,
                      const fqz5_filter_sums *d_sums);

/* Host restatement of the rule, one thread, no GPU: keep[r] (nrec bytes) = 1
 * where record r is selected, failed as above, sums (host arrays, may be
 * NULL) as above.  Every stream given is summed.  Fails as fqz5_filter_match
 * does. */
int fqz5_filter_host(const fqz5_filter_spec *, const uint8_t *seq, const uint8_t *qual,
                     uint64_t seq_len, const uint32_t *lens, uint64_t nrec, int pairs, int invert,
                     uint8_t *keep, uint64_t *failed, const fqz5_filter_sums *sums);

/* Trim and clip (trim.hip; fqz5file.trim_records / trim_file): per record the
 * interval of its bases and qualities that is kept, the cut points found on
 * the device, and the streams compacted to those intervals, after which they
 * are ordinary streams with new lengths (fqz5_filter_match judges them,
 * fqz5_fastq_format_list lays out their text).  Names are never trimmed.
 *
 * The rule is exact integer arithmetic, and the device and fqz5_trim_host
 * agree bit for bit.  A record has L bases s[0..L) and qualities q[0..L) (q
 * the quality line's byte - 33, as the decoder leaves it).  Its kept interval
 * [a, b) starts as [0, L) and goes through five steps in this order; a step
 * whose bit (below) is not in `set` does nothing, and every step leaves
 * a <= b:
 *   0 clip     a = min(head, L); b = max(a, L - min(tail, L))
 *   1 quality  both ends are judged on the interval [a0, b0) step 0 left,
 *              independently, by the running-sum rule of BWA and cutadapt:
 *                3' end (cutoff q3): sum = 0, best = 0, stop = b0; for
 *                i = b0 - 1 down to a0: sum += q3 - q[i]; if sum < 0 the scan
 *                ends; if sum > best (strictly: a tie keeps the larger i):
 *                best = sum, stop = i
 *                5' end (cutoff q5): start = a0; for i = a0 upwards:
 *                sum += q5 - q[i]; sum < 0 ends the scan; sum > best:
 *                best = sum, start = i + 1
 *              (an end whose cutoff is not set: start = a0, stop = b0); then
 *              a = start, b = max(start, stop).  Sums are i64.
 *   2 adapter  the smallest p in [a, b - min_overlap] at which some adapter
 *              matches; then b = p.  Adapter A of m bytes matches at p when,
 *              with ov = min(m, b - p), ov >= min_overlap and the positions
 *              0 <= k < ov with s[p + k] != A[k] number at most
 *              (max_err_pct * ov) / 100 (integer division).  Bytes are
 *              compared as they are: no case folding, no wildcard.  Of several
 *              adapters that match at the smallest p the lowest index counts.
 *   3 trim_n   while a < b and s[a] is in "Nn": a++; while b > a and s[b - 1]
 *              is in "Nn": b--
 *   4 crop     b = min(b, a + max_len)
 * With pairs, records 2k and 2k + 1 are each trimmed on their own; the odd
 * ones take the mate-2 adapters when there are any, else mate 1's.
 *
 * Counts (u64 words, added to): [0] bases_in, [1] bases_out, the bases of all
 * records before and after; [2 + k] trimmed[k], the records step k shortened;
 * [7 + k] removed[k], the bases step k took off; [12 + j] adapter_hits[j], the
 * records cut by the adapter in slot j. */
#define FQZ5_TRIM_STEPS 5
#define FQZ5_TRIM_ADAPTERS 16                 /* per mate */
#define FQZ5_TRIM_ADAPTER_MAX 128             /* bytes of one adapter */
#define FQZ5_TRIM_COUNTS (12 + 2 * FQZ5_TRIM_ADAPTERS)
#define FQZ5_TRIM_CLIP 1u
#define FQZ5_TRIM_Q5 2u
#define FQZ5_TRIM_Q3 4u
#define FQZ5_TRIM_ADAPTER 8u
#define FQZ5_TRIM_N 16u
#define FQZ5_TRIM_CROP 32u
typedef struct {
    uint32_t set;                 /* the FQZ5_TRIM_ bits of the steps that count */
    uint32_t q5, q3;              /* cutoffs, at most 93 */
    uint32_t min_overlap, max_err_pct;        /* >= 1; <= 100 */
    uint32_t n_adapters[2];       /* mate 1's, mate 2's (0: mate 1's serve both) */
    uint64_t head, tail, max_len;
} fqz5_trim_spec;

/* the adapters: mate 1's in slots 0 .. n_adapters[0] - 1, mate 2's after them;
 * each 1 .. FQZ5_TRIM_ADAPTER_MAX bytes */
typedef struct {
    uint32_t len[2 * FQZ5_TRIM_ADAPTERS];
    uint8_t bytes[2 * FQZ5_TRIM_ADAPTERS][FQZ5_TRIM_ADAPTER_MAX];
} fqz5_trim_adapters;

/* d_seq[0..seq_len) and d_qual[0..seq_len) (device) hold nrec records whose
 * lengths are h_len (host).  Per record its kept interval: where it starts
 * within the record into d_start (device, nrec words; stays there for
 * fqz5_trim_gather) and its length into h_new_len (host, nrec words); the
 * counts are added to h_counts (host, FQZ5_TRIM_COUNTS words).  `adapters` is
 * read only with the adapter step.  A stream that no step that is set reads
 * (the quality step: d_qual; adapter and trim_n: d_seq) is not read and may be
 * NULL.  Fails, before anything is written: a step without its stream, a
 * spec outside the limits above, lengths that do not sum to seq_len,
 * nrec >= 2^31, an odd nrec with pairs.  nrec 0: nothing is written. */
int fqz5_trim_cuts(const fqz5_trim_spec *, const fqz5_trim_adapters *adapters,
                   const uint8_t *d_seq, const uint8_t *d_qual, uint64_t seq_len,
                   const uint32_t *h_len, uint64_t nrec, int pairs, uint32_t *d_start,
                   uint32_t *h_new_len, uint64_t *h_counts);

/* One stream compacted: bytes [start, start + new_len) of every record of
 * d_src[0..seq_len) (device; record lengths h_len) one after the other into
 * d_dst (device, dst_cap bytes), *out_len their number.  d_start: device,
 * h_new_len: host, as fqz5_trim_cuts leaves them.  Source and destination are
 * distinct buffers: ranges that overlap fail, as do an interval outside its
 * record, lengths that do not sum to seq_len and a result above dst_cap
 * (h_new_len is checked against h_len on the host; d_start + new_len is
 * clipped to the record on the device, so no byte outside [0, seq_len) is
 * read). */
int fqz5_trim_gather(const uint8_t *d_src, uint64_t seq_len, const uint32_t *h_len,
                     const uint32_t *d_start, const uint32_t *h_new_len, uint64_t nrec,
                     uint8_t *d_dst, uint64_t dst_cap, uint64_t *out_len);

/* Host restatement of the rule, one thread, no GPU: start and new_len (nrec
 * words each), counts as above (added to), and, where given, the compacted
 * bases into out_seq and qualities into out_qual (the sum of new_len bytes
 * each; may be NULL).  Fails as fqz5_trim_cuts does. */
int fqz5_trim_host(const fqz5_trim_spec *, const fqz5_trim_adapters *adapters,
                   const uint8_t *seq, const uint8_t *qual, uint64_t seq_len,
                   const uint32_t *lens, uint64_t nrec, int pairs, uint32_t *start,
                   uint32_t *new_len, uint64_t *counts, uint8_t *out_seq, uint8_t *out_qual);

/* Duplicates (dedup.hip; fqz5file.dedup_records / dedup_file / duplication):
 * which records of a file are the first of their sequence.  A unit is one
 * record, with pairs the records 2k and 2k + 1 of a block.  A unit is kept
 * when no earlier unit of the file has the same key; invert selects exactly
 * the others.  Two units are duplicates when their 128-bit keys are equal:
 * equal sequences always, unequal sequences with probability about 2^-128 per
 * pair of units.
 *
 * A unit's key is a pair of u64 words, each a sum mod 2^64 of one term per
 * (position, byte) of its bases and one term for its length, so a record
 * spread over several tiles is summed tile by tile, in any order, to the same
 * bits; the device, fqz5_dedup_keys_host and tests/dedup_ref.py agree bit for
 * bit.  With
 *     mix(x):  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 *              x *= 0x94D049BB133111EB; x ^= x >> 31          (all u64)
 *     K_s(rec) = mix(SEED_s ^ L) + sum over i of mix(SEED_s + (i << 8 | c_i))
 * (L the record's length, c_i its i-th byte as it is: no case folding) and
 * the four odd seeds below:
 *     a record                  (K_0, K_1)
 *     pairs                     (K_0(R1) + K_2(R2), K_1(R1) + K_3(R2))
 *     revcomp                   the smaller of the record's key and its reverse
 *                               complement's, compared first word, then second;
 *                               the reverse complement's sums have
 *                               mix(SEED_s + ((L - 1 - i) << 8 | comp(c_i))) for
 *                               byte i, comp swapping A<->T and C<->G in either
 *                               case and leaving every other byte alone
 *     revcomp with pairs        the smaller of key(R1, R2) and key(R2, R1); no
 *                               base is complemented (the other strand of a
 *                               fragment shows up as swapped mates)
 *
 * The table: open addressing, linear probing from home slot
 * (first word) & (slots - 1), slots a power of two >= max(8, 2 * units).  A
 * slot holds one key, the smallest unit number that carried it (`first`) and
 * how many units did (`count`, u32).  Inserting is wait-free: no lane waits
 * for another's store.  Every key word is a legal key word, zero and all ones
 * included (an empty slot is told apart by bits of its own).  Unit numbers are
 * the caller's (first_unit + the unit's index in the call); a file's blocks
 * are given in file order, so `first` is final once the block is judged. */
#define FQZ5_DEDUP_SEED0 0x9E3779B97F4A7C15ull
#define FQZ5_DEDUP_SEED1 0xC2B2AE3D27D4EB4Full
#define FQZ5_DEDUP_SEED2 0x165667B19E3779F9ull
#define FQZ5_DEDUP_SEED3 0xD6E8FEB86659FD93ull
#define FQZ5_DEDUP_LEVELS 1025                /* counts 0..1023, then 1024 and more */
#define FQZ5_DEDUP_LEVEL_WORDS (FQZ5_DEDUP_LEVELS + 2)
typedef struct fqz5_dedup_table fqz5_dedup_table;
typedef struct fqz5_dedup_host_table fqz5_dedup_host_table;

/* the device bytes of a table for `units` units (0: more than 2^31 slots) */
uint64_t fqz5_dedup_table_bytes(uint64_t units);
/* A new, empty table for `units` units (NULL with fqz5_last_error() set: more
 * than 2^31 slots, no memory); its slots; emptied again. */
fqz5_dedup_table *fqz5_dedup_table_new(uint64_t units);
void fqz5_dedup_table_free(fqz5_dedup_table *);
uint64_t fqz5_dedup_table_slots(const fqz5_dedup_table *);
int fqz5_dedup_table_reset(fqz5_dedup_table *);
/* one slot as it stands: out[0..4) = key words, first, count (count 0: empty) */
int fqz5_dedup_table_slot(const fqz5_dedup_table *, uint64_t slot, uint64_t *out);

/* The unit keys of a block: d_seq[0..seq_len) (device) holds nrec records
 * whose lengths are h_len (host); unit u's key goes to d_keys[2u], [2u + 1]
 * (device, 2 * units words).  Fails, before anything is written: lengths that
 * do not sum to seq_len, nrec >= 2^31, an odd nrec with pairs. */
int fqz5_dedup_keys(const uint8_t *d_seq, uint64_t seq_len, const uint32_t *h_len, uint64_t nrec,
                    int pairs, int revcomp, uint64_t *d_keys);
/* n keys (device, as above) inserted as the units first_unit ..; d_slot
 * (device, n words) receives each one's slot.  Fails with "table full" when a
 * key finds no slot within `slots` probes (the table then holds some of the
 * call's keys: reset it). */
int fqz5_dedup_insert_keys(fqz5_dedup_table *, const uint64_t *d_keys, uint64_t n,
                           uint64_t first_unit, uint32_t *d_slot);
/* One block: its keys, their insertion as units first_unit .., and the
 * selected records' indices, ascending, into d_rec (device, nrec entries; both
 * mates of a selected pair), *n_hit their number.  d_first (device, one u64
 * per unit, may be NULL): the number of the first unit with the unit's key.
 * Fails as fqz5_dedup_keys and fqz5_dedup_insert_keys do. */
int fqz5_dedup_match(fqz5_dedup_table *, const uint8_t *d_seq, uint64_t seq_len,
                     const uint32_t *h_len, uint64_t nrec, int pairs, int revcomp, int invert,
                     uint64_t first_unit, uint32_t *d_rec, uint64_t *n_hit, uint64_t *d_first);
/* The table's duplication levels into h_out (host, FQZ5_DEDUP_LEVEL_WORDS
 * words): [c] the keys carried by c units for c < 1024, [1024] those carried by
 * 1024 and more, [1025] the keys, [1026] the largest count. */
int fqz5_dedup_levels(const fqz5_dedup_table *, uint64_t *h_out);

/* Host restatement, one thread, no GPU: the keys (2 * units words), and a
 * table (std::unordered_map on the 128-bit key) that takes n keys as the units
 * first_unit .. and leaves keep[u] (n bytes, may be NULL) = 1 where unit u is
 * selected and first[u] (n words, may be NULL); its levels as above. */
int fqz5_dedup_keys_host(const uint8_t *seq, uint64_t seq_len, const uint32_t *lens, uint64_t nrec,
                         int pairs, int revcomp, uint64_t *keys);
fqz5_dedup_host_table *fqz5_dedup_host_new(void);
void fqz5_dedup_host_free(fqz5_dedup_host_table *);
int fqz5_dedup_host_add(fqz5_dedup_host_table *, const uint64_t *keys, uint64_t n,
                        uint64_t first_unit, int invert, uint8_t *keep, uint64_t *first);
int fqz5_dedup_host_levels(const fqz5_dedup_host_table *, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif
