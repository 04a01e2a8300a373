// lime_seqcut_kernel.hip -- where to cut a window of a reads file so that whole records stand in front of the cut (lime_reader.cpp
// sequences the passes and reads a file in batches of records with them; include/lime_hip.h states the rule at lime_seq_cut_dev).
// The window b[0 .. n) begins at a record start, or is the file's first window; eof: it ends at the file's end.  A marker is
//   FASTQ  an '\n';   FASTA  a line-first '>': byte i is '>' and (i == 0 or b[i - 1] == '\n').
// With T the number of markers, the cut, the records m in front of it and T come out as three 64-bit words:
//   FASTQ  eof and T / 4 < max_reads:  cut = n, m = n_lines / 4 (n_lines = T, + 1 if n > 0 and b[n - 1] != '\n': what the parser will find);
//          else m = min(max_reads, T / 4) and cut = 1 + the position of marker 4m - 1 (markers count from 0); m == 0: cut = 0
//   FASTA  m = min(max_reads, eof ? T : max(T, 1) - 1);  eof and m == T: cut = n;  else cut = the position of marker m (T == 0: cut = 0)
// The passes over the blocks of LIME_FASTA_BLOCK bytes, a lane on 16 consecutive bytes, as in the two parser files:
//   1  the markers per block: k_fq_lines of lime_fastq_kernel.hip, launched as it is, or k_sc_headers here.
//      One exclusive prefix sum (rocPRIM, lime_index_sort.hip) over n_blocks + 1 entries: every block's first marker number, and T.
//   2  k_sc_select  every workgroup computes m and the wanted marker from T; the one block whose range of marker numbers holds it reads
//                   its bytes again, finds the lane and the bit, and that lane writes the three words.  Where no marker is wanted
//                   (cut = 0 or n) thread 0 of block 0 writes them.  Exactly one lane of the grid writes.
// The block geometry (BY_*), load_piece, the line-first mask and the sum over the waves (add_waves) are lime_bytes.h's.
// wave64.  The only cross-lane operation is the DPP prefix sum of lime_wave.h, in wave-uniform control flow: a workgroup skips a block as
// a whole (a condition on the block's number and the prefix sums alone), and every lane of it runs the blocks it does not skip; a lane
// past the end holds no bytes.  No inline assembly here, plain vector stores.  No byte outside [0, n) is loaded: a 16-byte load is issued
// only where all 16 bytes are inside, the byte in front of a lane's piece only where its position is > 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_wave.h"
#include "lime_bytes.h"

namespace lime {

namespace {

// bit j: byte j of the lane's piece is a marker of `format` (0 FASTA, 1 FASTQ).  The byte in front of the piece is read for FASTA only.
// (lime_bytes.h's byte_masks gives the same masks; built on it, these two kernels come out as other code, so the two masks are made here)
__device__ __forceinline__ uint32_t piece_markers(const uint8_t *b, uint64_t n, uint64_t pos, int format)
{
    uint32_t w[4];
    const uint32_t len = load_piece(b, n, pos, w);
    uint32_t nl = 0u, gt = 0u;
#pragma unroll
    for (uint32_t j = 0; j < BY_LANE; ++j) {
        nl |= (uint32_t)(byte_of(w, j) == '\n') << j;
        gt |= (uint32_t)(byte_of(w, j) == '>') << j;
    }
    const uint32_t in = (1u << len) - 1u;                                   // (len <= 16)
    nl &= in; gt &= in;
    return format ? nl : line_first(b, pos, len, nl) & gt;
}

// ---- pass 1, FASTA ----
__global__ void __launch_bounds__(BY_WG) k_sc_headers(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *cnt)
{
    __shared__ uint32_t s_sum[BY_WAVES];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t pos = (uint64_t)blk * LIME_FASTA_BLOCK + threadIdx.x * BY_LANE;
        const uint32_t incl = wave_incl_scan((uint32_t)__builtin_popcount(piece_markers(b, n, pos, 0)));
        if (lane == 63u) s_sum[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) cnt[blk] = add_waves(s_sum, BY_WAVES);
        __syncthreads();
    }
}

// ---- pass 2 ----
// off: the exclusive sum of pass 1's counts over n_blocks + 1 entries (off[n_blocks] = T).  n > 0, n_blocks = ceil(n / LIME_FASTA_BLOCK).
__global__ void __launch_bounds__(BY_WG) k_sc_select(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *off, int format, uint32_t max_reads,
                                                     int eof, unsigned long long *out)
{
    __shared__ uint32_t s_sum[BY_WAVES];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t T = (uint32_t)__builtin_amdgcn_readfirstlane((int)off[n_blocks]);
    // m, and the wanted marker (want = 0: none, the cut is `fixed`)
    uint32_t m, marker = 0u, want = 0u;
    uint64_t fixed = 0;
    if (format) {
        if (eof && T / 4u < max_reads) {
            m = (T + (uint32_t)__builtin_amdgcn_readfirstlane((int)(b[n - 1] != '\n'))) / 4u;
            fixed = n;
        } else {
            m = T / 4u < max_reads ? T / 4u : max_reads;
            if (m) { want = 1u; marker = 4u * m - 1u; }
        }
    } else {
        const uint32_t avail = eof ? T : (T ? T - 1u : 0u);
        m = avail < max_reads ? avail : max_reads;
        if (eof && m == T) fixed = n;
        else if (T) { want = 1u; marker = m; }
    }
    if (!want) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = fixed; out[1] = m; out[2] = T; }
        return;
    }
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        // (the same for every lane of the workgroup, and known to the compiler as such: the skip is a scalar branch)
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)off[blk]), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)off[blk + 1u]);
        if (marker < lo || marker >= hi) continue;
        const uint64_t pos = (uint64_t)blk * LIME_FASTA_BLOCK + threadIdx.x * BY_LANE;
        const uint32_t mk = piece_markers(b, n, pos, format);
        const uint32_t mine = (uint32_t)__builtin_popcount(mk), incl = wave_incl_scan(mine);
        if (lane == 63u) s_sum[wave] = incl;
        __syncthreads();
        const uint32_t before = add_waves(s_sum, wave, lo + incl - mine);   // the number of the piece's first marker
        if (marker >= before && marker < before + mine) {
            uint32_t rest = mk;                  // drop the markers in front of the wanted one: its bit is then the lowest
            for (uint32_t k = before; k < marker; ++k) rest &= rest - 1u;
            out[0] = pos + (uint32_t)__builtin_ctz(rest) + (format ? 1u : 0u);
            out[1] = m;
            out[2] = T;
        }
        __syncthreads();
    }
}

} // namespace

void sc_launch_headers(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *cnt, hipStream_t st)
{
    if (n_blocks) k_sc_headers<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, cnt);
}

void sc_launch_select(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *off, int format, uint32_t max_reads, int eof, uint64_t *out,
                      hipStream_t st)
{
    if (n_blocks)
        k_sc_select<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, off, format, max_reads, eof, (unsigned long long *)out);
}

} // namespace lime
