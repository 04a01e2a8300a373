// lime_fastq_kernel.hip -- four-line FASTQ bytes to documents on the device (lime_docs.cpp sequences the passes; include/lime_hip.h states
// what lime_fastq_read, the oracle, returns and refuses).  Records are found by counting lines, never by looking for '@': a quality
// string may begin with '@' or '+'.  The rule per byte, for the input b[0 .. n):
//   ln(i)                  the number of '\n' in b[0 .. i): an '\n' belongs to the line it ends
//   byte i is line-first   iff i == 0 or b[i - 1] == '\n'
//   n_lines                the number of '\n', + 1 if n > 0 and b[n - 1] != '\n'
//   byte i is kept         iff ln(i) % 4 == 1 and b[i] is neither '\n' nor '\r';   it is a quality byte iff the same holds with ln(i) % 4 == 3
//   text = the kept bytes in order;  document k starts at the number of kept bytes before the line-first byte of line 4k;
//   n_docs = n_lines / 4, doc_off[n_docs] = the number of kept bytes
// Refused, as min over all offences of line * 4 + reason (lines count from 1; one 64-bit atomicMin, so the answer does not depend on the
// order the blocks run in):
//   0  the line-first byte of a line 4k is not '@'         1  the line-first byte of a line 4k + 2 is not '+'
//   2  at a record's end (the '\n' that ends a line 4k + 3, or the last input byte where it lies on such a line and is no '\n') the kept bytes
//      so far and the quality bytes so far differ in number: the lowest such line is the lowest line whose length differs from its sequence's
//   3  n_lines % 4 != 0, at line n_lines
// The input is cut into blocks of LIME_FASTA_BLOCK bytes, one workgroup pass each, a lane on 16 consecutive bytes, as in lime_fasta_kernel.hip:
//   1  k_fq_lines   per block the number of '\n'.  One exclusive prefix sum (rocPRIM, lime_index_sort.hip) gives every block the line number
//                   of its first byte, and the total.
//   2  k_fq_count   per block the kept bytes and the kept bytes minus the quality bytes (modulo 2^32); reasons 0 and 1 at the line-first
//                   bytes; n_lines and reason 3 by the lane that holds the last input byte.  One exclusive prefix sum each.
//   3  k_fq_write   the kept bytes through LDS to their places with 16-byte stores, the doc_off entries, and reason 2 at the record ends.
// The line-first byte of line 4k is record start k whatever the block: no count of record starts crosses blocks (document k's entry is
// written by the lane that holds that byte, at index ln / 4).  Passes 2 and 3 build the same masks (block_marks): 3 reads per input
// byte and 1 write per kept byte, which are fewer than half of the bytes.
// block_marks, with the rule above in code, is lime_fastq_marks.h's (the quality pass of lime_fqtrim_kernel.hip takes its mask from it too); the block
// geometry (BY_*), load_piece, the per-byte masks, the sum over the waves (add_waves) and the write-out (store_staged) are lime_bytes.h's.
// wave64.  The only cross-lane operations are the DPP prefix sum of lime_wave.h, in wave-uniform control flow (every lane of a
// workgroup runs every block of its stride loop; a lane past the end holds no bytes).  No inline assembly here, plain vector stores.
// No byte outside [0, n) is loaded: a 16-byte load is issued only where all 16 bytes are inside, the byte in front of a lane's piece
// only where its position is > 0.  Every store is inside text[0 .. kept bytes) and doc_off[0 .. n_docs], valid input or not.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_wave.h"
#include "lime_bytes.h"
#include "lime_fastq_marks.h"

namespace lime {

namespace {

// ---- pass 1 ----
__global__ void __launch_bounds__(BY_WG) k_fq_lines(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *cnt_lf)
{
    __shared__ uint32_t s_sum[BY_WAVES];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t pos = (uint64_t)blk * LIME_FASTA_BLOCK + threadIdx.x * BY_LANE;
        uint32_t w[4];
        const uint32_t len = load_piece(b, n, pos, w);
        uint32_t nl = 0u;
#pragma unroll
        for (uint32_t j = 0; j < BY_LANE; ++j) nl += (uint32_t)(j < len && byte_of(w, j) == '\n');
        const uint32_t incl = wave_incl_scan(nl);
        if (lane == 63u) s_sum[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) cnt_lf[blk] = add_waves(s_sum, BY_WAVES);
        __syncthreads();
    }
}

// ---- passes 2 and 3: the masks of a block are block_marks of lime_fastq_marks.h ----
// kept bytes in the low half, quality bytes in the high half: a block has at most 4096 of each
__device__ __forceinline__ uint32_t packed_counts(const Marks &m) { return (uint32_t)__builtin_popcount(m.keep) | ((uint32_t)__builtin_popcount(m.qual) << 16); }

// *err = min(itself, line * 4 + reason) over reasons 0, 1 and 3; *n_lines is written
__global__ void __launch_bounds__(BY_WG) k_fq_count(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, uint32_t *cnt_keep, uint32_t *cnt_diff,
                                                    unsigned long long *err, uint32_t *n_lines)
{
    __shared__ uint32_t s_lf[BY_WAVES], s_sum[BY_WAVES];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        Piece p;
        const Marks m = block_marks(b, n, blk, line0, s_lf, p);
        const uint32_t incl = wave_incl_scan(packed_counts(m));
        if (lane == 63u) s_sum[wave] = incl;
        if (m.bad) {                             // a line has one line-first byte: the lowest bit is the lowest line
            const uint32_t j = (uint32_t)__builtin_ctz(m.bad);
            atomicMin(err, line_of(p, m, j) * 4u + ((m.bad1 >> j) & 1u));
        }
        const uint64_t pos = (uint64_t)blk * LIME_FASTA_BLOCK + threadIdx.x * BY_LANE;
        if (p.len && pos + p.len == n) {         // the lane of the last input byte: the total of pass 1 stands behind the last block's entry
            const uint32_t lines = line0[n_blocks] + (((p.nl >> (p.len - 1u)) & 1u) ^ 1u);
            *n_lines = lines;
            if (lines & 3u) atomicMin(err, (unsigned long long)lines * 4u + 3u);
        }
        __syncthreads();                         // (the only one of its own: block_marks' stands between this block's reads of s_sum and the next one's post)
        if (threadIdx.x == 0) {
            const uint32_t t = add_waves(s_sum, BY_WAVES);
            cnt_keep[blk] = t & 0xFFFFu;
            cnt_diff[blk] = (t & 0xFFFFu) - (t >> 16);
        }
    }
}

// off_keep / off_diff: the exclusive sums of pass 2's counts, n_blocks + 1 entries (the last one the total); n_docs = n_lines / 4
__global__ void __launch_bounds__(BY_WG) k_fq_write(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, const uint32_t *off_keep,
                                                    const uint32_t *off_diff, uint32_t n_docs, uint8_t *text, uint64_t *doc_off, unsigned long long *err)
{
    __shared__ uint32_t s_lf[BY_WAVES], s_sum[BY_WAVES];
    __shared__ uint4 s_stage[LIME_FASTA_BLOCK / 16 + 1];                    // the block's kept bytes, placed as in `text` modulo 16
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_stage);
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        Piece p;
        const Marks m = block_marks(b, n, blk, line0, s_lf, p);
        const uint32_t mine = packed_counts(m), incl = wave_incl_scan(mine);
        if (lane == 63u) s_sum[wave] = incl;
        __syncthreads();
        // kept bytes | quality bytes of the block in front of this piece, and of the block
        const uint32_t before = add_waves(s_sum, wave, incl - mine), total = add_waves(s_sum, BY_WAVES);
        const uint32_t base = off_keep[blk], shift = base & 15u, n_keep = total & 0xFFFFu;
        uint32_t at = shift + (before & 0xFFFFu);
#pragma unroll
        for (uint32_t j = 0; j < BY_LANE; ++j)
            if ((m.keep >> j) & 1u) stage[at++] = (uint8_t)(p.w[j >> 2] >> ((j & 3u) * 8u));
        for (uint32_t rs = m.rs; rs; rs &= rs - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(rs);
            const uint64_t doc = (line_of(p, m, j) - 1u) >> 2;              // (< n_docs unless the last record is truncated)
            if (doc < n_docs) doc_off[doc] = (uint64_t)base + (before & 0xFFFFu) + (uint32_t)__builtin_popcount(m.keep & ((1u << j) - 1u));
        }
        // kept bytes minus quality bytes of b[0 .. the record's end], modulo 2^32: both counts are below 2^32
        const uint32_t diff = off_diff[blk] + (before & 0xFFFFu) - (before >> 16);
        for (uint32_t e = m.end; e; e &= e - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(e), upto = (2u << j) - 1u;
            if (diff + (uint32_t)__builtin_popcount(m.keep & upto) - (uint32_t)__builtin_popcount(m.qual & upto) != 0u) {
                atomicMin(err, line_of(p, m, j) * 4u + 2u);
                break;                           // (the piece's later ends are higher lines)
            }
        }
        __syncthreads();
        store_staged(s_stage, text + (base - shift), shift, n_keep);       // stage[shift .. shift + n_keep) to text[base ..); text is 16-byte aligned
        if (blk == n_blocks - 1u && threadIdx.x == 0) doc_off[n_docs] = off_keep[n_blocks];
        __syncthreads();
    }
}

} // namespace

void fq_launch_lines(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *cnt_lf, hipStream_t st)
{
    if (n_blocks) k_fq_lines<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, cnt_lf);
}

void fq_launch_count(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, uint32_t *cnt_keep, uint32_t *cnt_diff, uint64_t *err,
                     uint32_t *n_lines, hipStream_t st)
{
    if (n_blocks) k_fq_count<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, line0, cnt_keep, cnt_diff, (unsigned long long *)err, n_lines);
}

void fq_launch_write(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, const uint32_t *off_keep, const uint32_t *off_diff,
                     uint32_t n_docs, uint8_t *text, uint64_t *doc_off, uint64_t *err, hipStream_t st)
{
    if (n_blocks)
        k_fq_write<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, line0, off_keep, off_diff, n_docs, text, doc_off, (unsigned long long *)err);
}

} // namespace lime
