// lime_index.h -- what the index builder's three parts share: the kernels (lime_index_kernel.hip), the rocPRIM sorts and
// prefix sums (lime_index_sort.hip, a translation unit of its own) and the host sequencing (lime_build.cpp: build_index_impl), and
// the kernels of the merge into a prebuilt genome index (lime_merge_kernel.hip; host sequencing in lime_merge.cpp).
// Not part of the public ABI (include/lime_hip.h is).
//
// Positions: the collection with one terminator after every document has N = n_text + n_docs positions; document k owns
// [doc_off[k] + k, doc_off[k + 1] + k], the last one its terminator.  The symbol at a non-terminator position p of document k is
// text[p - k].  A suffix is named by its position (u32: N <= 2^32 - 1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"                                    // (lime_filter_t)

namespace lime {

constexpr uint32_t IDX_STRETCH = 16;             // consecutive positions one lane of k_idx_lcp walks (Kasai's bound carried along)

struct IdxText {                                 // the collection as the kernels see it
    const uint8_t *text;                         // n_text symbols, no terminators
    const uint64_t *doc_off;                     // [n_docs + 1]
    const uint32_t *doc_of;                      // [N] document of every position
    uint64_t n_text;
    uint32_t n_docs, n;                          // n = N
};

// ---- lime_index_kernel.hip ----
// err |= 1 unless doc_off[0] == 0, doc_off is non-decreasing and doc_off[n_docs] == n_text; present[b] = 1 for every byte b of the text
void idx_launch_check(const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, const uint8_t *text, uint32_t *present, uint32_t *err, hipStream_t st);
// code[b] = 1 + number of present bytes below b (0 for absent bytes); *sigma = number of present bytes
void idx_launch_codes(const uint32_t *present, uint16_t *code, uint32_t *sigma, hipStream_t st);
// flags[doc_off[k] + k] = 1 for k = 1 .. n_docs - 1 (flags zeroed by the caller; its inclusive sum is doc_of)
void idx_launch_doc_heads(const uint64_t *doc_off, uint32_t n_docs, uint32_t *flags, hipStream_t st);
// keys[p] = the first k_syms symbols' codes of suffix p, `bits` each, first symbol highest; 0 from the terminator on.  vals[p] = p
void idx_launch_pack(const IdxText &t, const uint16_t *code, uint32_t k_syms, uint32_t bits, uint64_t *keys, uint32_t *vals, hipStream_t st);
// element j of a sorted list of m (key, suffix) pairs that sits at suffix-array slot idx[j] (idx NULL: slot j).  A new group starts at
// j == 0, where the key changes, and (low_mask != 0) where key & low_mask == 0: the terminator is inside the packed window, the suffix
// is alone.  head_pos[j] = the slot if j starts a group, else 0 (its running maximum is every element's group head)
void idx_launch_heads(const uint64_t *keys, const uint32_t *idx, uint32_t m, uint64_t low_mask, uint32_t *head_pos, hipStream_t st);
// rank[vals[j]] = grp[j], sa[slot j] = vals[j] (both arrays of n), act[j] = 1 unless j is a group of one
void idx_launch_settle(const uint64_t *keys, const uint32_t *vals, const uint32_t *idx, const uint32_t *grp, uint32_t m, uint64_t low_mask,
                       uint32_t n, uint32_t *rank, uint32_t *sa, uint32_t *act, hipStream_t st);
// the elements with act[j] != 0 move to slot pos[j] of (idx_out, vals_out)
void idx_launch_compact(const uint32_t *vals, const uint32_t *idx, const uint32_t *act, const uint32_t *pos, uint32_t m,
                        uint32_t *vals_out, uint32_t *idx_out, hipStream_t st);
// keys[j] = rank[vals[j]] << nb | rank[vals[j] + h]
void idx_launch_double(const uint32_t *vals, uint32_t m, const uint32_t *rank, uint32_t n, uint64_t h, uint32_t nb, uint64_t *keys, hipStream_t st);
// da[i] = doc_of[sa[i]], ebwt[i] = the symbol before suffix sa[i] (term for a document's whole suffix); either may be NULL
void idx_launch_gather(const IdxText &t, const uint32_t *sa, uint8_t term, uint32_t *da, uint8_t *ebwt, hipStream_t st);
// lcp[rank[p]] for every position p (rank = the inverse of sa), capped at lcp_cap when that is not 0
void idx_launch_lcp(const IdxText &t, const uint32_t *sa, const uint32_t *rank, uint32_t lcp_cap, uint32_t *lcp, hipStream_t st);

// ---- lime_merge_kernel.hip: read suffixes merged into a prebuilt genome index (lime_merge_index_dev, lime_merge.cpp) ----
// One side of the merge as its kernels see it: a collection of its own (positions and doc_off count from 0 on each side) with its suffix
// array and the document of every slot.  Every kernel clamps sa[s] to < n, da[s] to < n_docs and the position into its document, so a
// genome index loaded from a damaged file gives wrong output and no read outside text / doc_off.
struct MrgSide {
    const uint8_t *text;                         // n_text symbols, no terminators
    const uint64_t *doc_off;                     // [n_docs + 1], checked (k_idx_check / lime_gindex_load) before any of these kernels runs
    const uint32_t *sa, *da;                     // [n] suffix position and its document, in sorted order
    const uint8_t *ebwt;                         // [n] (may be NULL when no ebwt is asked for)
    const uint32_t *lcp;                         // [n] lcp with the slot before on this side (may be NULL when no lcp is asked for)
    uint64_t n_text;
    uint32_t n_docs, n;
};
// j[i] = number of genome suffixes below read suffix i (i in the reads' sorted order): a lower bound over g.sa by text comparison.
// Symbols compare as unsigned bytes, a suffix that ends is below one that goes on, and of two that end together the read is below.
void mrg_launch_rank(const MrgSide &r, const MrgSide &g, uint32_t *j, hipStream_t st);
// end[j[i]] = i + 1 wherever j[i] != j[i + 1] or i is the last read suffix (end: g.n + 1 words zeroed by the caller; its running maximum
// is c[k] = number of read suffixes with j <= k); *runs += the number of such i
void mrg_launch_ends(const uint32_t *j, uint32_t nr, uint32_t ng, uint32_t *end, uint32_t *runs, hipStream_t st);
// read suffix i goes to slot i + j[i], genome suffix k to slot k + c[k]: da (the genomes' ids + n_reads), ebwt and lcp of the merged
// order; lcp from the side's own array where the slot before is of the same side, else compared from the two texts; capped at lcp_cap
// when that is not 0.  Any output may be NULL.
void mrg_launch_write_reads(const MrgSide &r, const MrgSide &g, const uint32_t *j, uint32_t lcp_cap, uint8_t *ebwt, uint32_t *lcp, uint32_t *da, hipStream_t st);
void mrg_launch_write_genomes(const MrgSide &r, const MrgSide &g, const uint32_t *c, uint32_t lcp_cap, uint8_t *ebwt, uint32_t *lcp, uint32_t *da, hipStream_t st);

// ---- lime_fasta_kernel.hip: FASTA bytes to documents, reverse complements (lime_docs.cpp) ----
// The input b[0 .. n), n < 2^32, in n_blocks = ceil(n / LIME_FASTA_BLOCK) blocks; the rule per byte is at the head of the kernel file.
// last_lf[k] = 1 + the last line-first position of block k (0: none); *first_hdr = min(itself, the first line-first '>')
void fa_launch_lines(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *last_lf, uint32_t *first_hdr, hipStream_t st);
// cum_lf = the running maximum of last_lf.  cnt_keep[k], cnt_hdr[k] = kept bytes and header starts of block k
void fa_launch_count(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *cum_lf, const uint32_t *first_hdr, uint32_t *cnt_keep, uint32_t *cnt_hdr,
                     hipStream_t st);
// off_keep, off_hdr = the exclusive sums of the counts over n_blocks + 1 entries (a 0 appended: the last entry is the total).
// text (16-byte aligned, off_keep[n_blocks] bytes) and doc_off[off_hdr[n_blocks] + 1] are written, every byte and entry once
void fa_launch_write(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *cum_lf, const uint32_t *first_hdr, const uint32_t *off_keep,
                     const uint32_t *off_hdr, uint8_t *text, uint64_t *doc_off, hipStream_t st);
// *err = 1 unless doc_off[0] == 0, doc_off never decreases and doc_off[n_docs] == n_text
void fa_launch_check_off(const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, uint32_t *err, hipStream_t st);
// out[doc_off[d] + k] = comp[in[doc_off[d + 1] - 1 - k]]; out 16-byte aligned, doc_off checked
void fa_launch_revcomp(const uint8_t *in, const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, uint8_t *out, hipStream_t st);

// ---- lime_fastq_kernel.hip: four-line FASTQ bytes to documents (lime_docs.cpp) ----
// The same blocks; the rule per byte and the refusals are at the head of the kernel file.  cnt_lf[k] = the '\n' of block k
void fq_launch_lines(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *cnt_lf, hipStream_t st);
// line0 = the exclusive sum of cnt_lf over n_blocks + 1 entries (a 0 appended).  cnt_keep[k], cnt_diff[k] = kept bytes, and kept minus quality
// bytes modulo 2^32, of block k; *n_lines; *err = min(itself, line * 4 + reason) over the offences of reasons 0, 1 and 3 (lines from 1)
void fq_launch_count(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, uint32_t *cnt_keep, uint32_t *cnt_diff, uint64_t *err,
                     uint32_t *n_lines, hipStream_t st);
// off_keep, off_diff = the exclusive sums of the counts over n_blocks + 1 entries.  text (16-byte aligned, off_keep[n_blocks] bytes) and
// doc_off[n_docs + 1], n_docs = n_lines / 4, are written, every byte and entry once if the input is valid, never out of bounds if it is
// not; *err takes reason 2 the same way
void fq_launch_write(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, const uint32_t *off_keep, const uint32_t *off_diff,
                     uint32_t n_docs, uint8_t *text, uint64_t *doc_off, uint64_t *err, hipStream_t st);

// ---- lime_fqtrim_kernel.hip: the quality bytes of a FASTQ parse, and the quality trim (lime_docs.cpp) ----
// The parse's fourth pass, behind fq_launch_count's prefix sums: the quality bytes in order to qual (16-byte aligned); only qual[0 .. cap)
// is written, whatever the input holds
void fqt_launch_qual(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, const uint32_t *off_keep, const uint32_t *off_diff, uint8_t *qual,
                     uint64_t cap, hipStream_t st);
// lo32[r], len32[r]: what the rule (include/lime_hip.h: lime_quality_trim) keeps of read r, text[doc_off[r] + lo32[r] .. + len32[r]);
// counts[0] += the reads it changes, counts[1] += the reads with symbols of which it keeps none.  q5, q3 <= 93
void fqt_launch_bounds(const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t q5, uint32_t q3, uint32_t *lo32, uint32_t *len32,
                       uint64_t *counts, hipStream_t st);
// new_off = the exclusive sum of len32 over n_docs + 1 entries (a 0 appended).  out (new_off[n_docs] bytes) and out_off[n_docs + 1] are written
void fqt_launch_copy(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const uint32_t *lo32, const uint32_t *len32, const uint32_t *new_off,
                     uint8_t *out, uint64_t *out_off, hipStream_t st);

// ---- lime_adapter_kernel.hip: where a 3' adapter begins in every read (lime_docs.cpp) ----
// lo32[r] = 0, len32[r] = what the rule (include/lime_hip.h: lime_adapter_trim) keeps of read r, in fqt_launch_bounds' conventions, so that
// the prefix sum and fqt_launch_copy follow unchanged; counts as there.  masks[b]: bit j set where the adapter's symbol j is "ACGT"[b];
// 1 <= min_overlap <= m <= 64, max_err_pct <= 50
void ad_launch_bounds(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const uint64_t masks[4], uint32_t m, uint32_t min_overlap,
                      uint32_t max_err_pct, uint32_t *lo32, uint32_t *len32, uint64_t *counts, hipStream_t st);

// ---- lime_filter_kernel.hip: what the read filter keeps of every read (lime_docs.cpp) ----
// lo32[r] = 0, len32[r] = what the rule (include/lime_hip.h: lime_read_filter) keeps of read r, in fqt_launch_bounds' conventions, so that
// the prefix sum and fqt_launch_copy follow unchanged.  counts[0 .. 5) += the reads with a poly-X tail, the reads the cap shortened, the
// reads emptied as short, for their N's, for their complexity.  *f as lime_read_filter accepts it
void fl_launch_bounds(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const lime_filter_t *f, uint32_t *lo32, uint32_t *len32, uint64_t *counts,
                      hipStream_t st);

// ---- lime_qc_kernel.hip: per-position statistics of the reads (lime_docs.cpp) ----
// tables[0 .. LIME_QC_WORDS(n_pos)) (device memory) += the counts of the rule (include/lime_hip.h: lime_read_qc); qual may be NULL: documents
// without qualities.  1 <= n_pos <= LIME_QC_MAX_POS; nothing is launched for no reads
void qc_launch_reads(const uint8_t *text, const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t n_pos, uint64_t *tables, hipStream_t st);

// ---- lime_overlap_kernel.hip: where the two mates of a pair run into the adapter, from their overlap alone (lime_docs.cpp) ----
// With I* of pair r by the rule (include/lime_hip.h: lime_pair_overlap_trim): lo1[r] = lo2[r] = 0, len1[r] = min(La, I*), len2[r] =
// min(Lb, I*) (La, Lb without an I*), in fqt_launch_bounds' conventions, so that per mate the prefix sum and fqt_launch_copy follow
// unchanged; insert32[r] = I* or 0 (insert32 may be NULL).  counts[0] += the pairs with an I*, counts[1] += the pairs of which a mate got
// shorter.  min_overlap >= 1, max_err_pct <= 50
void ov_launch_bounds(const uint8_t *text1, const uint64_t *doc_off1, const uint8_t *text2, const uint64_t *doc_off2, uint32_t n_docs, uint32_t min_overlap,
                      uint32_t max_err_pct, uint32_t *lo1, uint32_t *len1, uint32_t *lo2, uint32_t *len2, uint32_t *insert32, uint64_t *counts, hipStream_t st);

// ---- lime_seqcut_kernel.hip: where a window of a reads file is cut into whole records (lime_reader.cpp) ----
// The same blocks; the markers and the rule are at the head of the kernel file.  cnt[k] = the line-first '>' of block k (FASTQ counts
// its markers with fq_launch_lines)
void sc_launch_headers(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *cnt, hipStream_t st);
// off = the exclusive sum of the counts over n_blocks + 1 entries (a 0 appended).  out[0 .. 3) = the cut, the records in front of it, the
// window's markers: written by exactly one lane.  format: 0 FASTA, 1 FASTQ; n > 0
void sc_launch_select(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *off, int format, uint32_t max_reads, int eof, uint64_t *out,
                      hipStream_t st);

// ---- lime_index_sort.hip: rocPRIM's device primitives.  temp == NULL: only *temp_bytes is set (the size to pass next time) ----
struct IdxPairs { uint64_t *keys[2]; uint32_t *vals[2]; int cur; };       // double buffers; cur = which holds the data (updated by the sort)
hipError_t idx_sort_pairs(void *temp, size_t *temp_bytes, IdxPairs *b, size_t m, unsigned begin_bit, unsigned end_bit, hipStream_t st);
hipError_t idx_scan_sum(void *temp, size_t *temp_bytes, const uint32_t *in, uint32_t *out, size_t m, bool inclusive, hipStream_t st);
hipError_t idx_scan_sum64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, size_t m, hipStream_t st);      // exclusive
hipError_t idx_scan_max(void *temp, size_t *temp_bytes, const uint32_t *in, uint32_t *out, size_t m, hipStream_t st);

} // namespace lime
