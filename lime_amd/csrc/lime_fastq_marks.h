// lime_fastq_marks.h -- the masks of a block of four-line FASTQ bytes, for every pass that needs the line rule (lime_fastq_kernel.hip's count
// and write passes, lime_fqtrim_kernel.hip's quality pass); lime_fastq_kernel.hip states the rule per byte.  Built on lime_bytes.h's pieces.
#pragma once
#include "lime_bytes.h"

namespace lime {

typedef ByteMasks Piece;                         // with line-first; c0: byte j is '@', c1: it is '+'

struct Marks {
    uint32_t keep, qual;                         // bit j: byte j of the lane's piece is kept, is a quality byte
    uint32_t rs;                                 // a record start: the line-first byte of a line 4k
    uint32_t bad, bad1;                          // a line-first byte that breaks reason 0 or 1; of those, the ones that break reason 1
    uint32_t end;                                // a record's end
    uint32_t ln0;                                // ln of the piece's first byte
};

// the line number of byte j of a piece, counted from 1
__device__ __forceinline__ uint64_t line_of(const Piece &p, const Marks &m, uint32_t j) { return (uint64_t)m.ln0 + (uint32_t)__builtin_popcount(p.nl & ((1u << j) - 1u)) + 1u; }

// line0: the exclusive sum of the blocks' '\n' counts (line0[k] = ln of block k's first byte).  One __syncthreads inside; s_lf[BY_WAVES] is
// read before the caller's next one, so a caller with a barrier of its own per block may come straight back.
__device__ __forceinline__ Marks block_marks(const uint8_t *b, uint64_t n, uint32_t blk, const uint32_t *line0, uint32_t (&s_lf)[BY_WAVES], Piece &p)
{
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t pos = (uint64_t)blk * LIME_FASTA_BLOCK + threadIdx.x * BY_LANE;
    p = byte_masks(b, n, pos, true, '@', '+');
    const uint32_t mine = (uint32_t)__builtin_popcount(p.nl), incl = wave_incl_scan(mine);
    if (lane == 63u) s_lf[wave] = incl;
    __syncthreads();
    Marks m;
    m.ln0 = add_waves(s_lf, wave, line0[blk] + incl - mine);
    uint32_t is0 = 0u, is1 = 0u, is2 = 0u, is3 = 0u, c = m.ln0 & 3u;       // bit j: ln(byte j) % 4 is 0, 1, 2, 3
#pragma unroll
    for (uint32_t j = 0; j < BY_LANE; ++j) {
        is0 |= (uint32_t)(c == 0u) << j; is1 |= (uint32_t)(c == 1u) << j;
        is2 |= (uint32_t)(c == 2u) << j; is3 |= (uint32_t)(c == 3u) << j;
        c = (c + ((p.nl >> j) & 1u)) & 3u;
    }
    const uint32_t sym = p.in() & ~p.nl & ~p.cr;
    m.keep = is1 & sym;
    m.qual = is3 & sym;
    m.rs = p.lf & is0;
    m.bad1 = p.lf & is2 & ~p.c1;
    m.bad = (p.lf & is0 & ~p.c0) | m.bad1;
    const uint32_t last = p.len && pos + p.len == n ? 1u << (p.len - 1u) : 0u;   // the last input byte
    m.end = is3 & (p.nl | last);
    return m;
}

} // namespace lime
