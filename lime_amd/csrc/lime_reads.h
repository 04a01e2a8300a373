// lime_reads.h -- what the kernels that put one wave on a read share (lime_adapter_kernel.hip, lime_filter_kernel.hip, lime_qc_kernel.hip,
// lime_overlap_kernel.hip): the launch geometry, a lane's guarded byte of a read, the four base-class words of 64 symbols, and the walk of
// a wave over its reads, two ahead.  Device code (and the launchers' grid size); every function is inlined into its caller.  A read is
// text[doc_off[r] .. doc_off[r + 1]); lane i of word w holds symbol 64 w + i where it lies in the read.  No byte outside a read is loaded.
// wave64: the walk and whatever runs in it is wave-uniform control flow (blockIdx, the wave's index and the reads' bounds made scalar), so
// a ballot in the per-read work has every lane taking part, the lanes outside the read with no value.  No inline assembly, no LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_wave.h"

namespace lime {

constexpr int RD_WG = 256;
constexpr uint32_t RD_WAVES = RD_WG / 64;        // reads a workgroup handles per trip
constexpr uint32_t RD_BLOCKS = 2048;             // eight workgroups a CU: the grid is capped and the waves stride

// the grid for n_docs reads, 0 for none
inline uint32_t rd_grid(uint32_t n_docs)
{
    const uint64_t nb = ((uint64_t)n_docs + RD_WAVES - 1u) / RD_WAVES;
    return nb < RD_BLOCKS ? (uint32_t)nb : RD_BLOCKS;
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// byte `at` of the read s[0 .. L) as it is, 0 (no base) outside it.  Nothing is done to the byte here: a prefetched one is waited for
// where it is first used (base_words, as a rule), not where it is asked for
__device__ __forceinline__ uint32_t read_load(const uint8_t *s, uint64_t L, uint64_t at)
{
    return at < L ? (uint32_t)s[at] : 0u;
}

struct BaseWords { uint64_t b[4]; };             // R_A, R_C, R_G, R_T of 64 symbols: 0 bits behind the read's end and at what is no base

__device__ __forceinline__ BaseWords base_words(uint32_t c)
{
    BaseWords w;
    c &= 0xDFu;                                  // (lower case is its base)
    w.b[0] = __ballot(c == 'A'); w.b[1] = __ballot(c == 'C'); w.b[2] = __ballot(c == 'G'); w.b[3] = __ballot(c == 'T');
    return w;
}

// the k lowest bits, k in 0 .. 64 and above
__device__ __forceinline__ uint64_t low_bits(uint64_t k)
{
    return k >= 64u ? ~0ull : (1ull << k) - 1u;
}

// The wave's reads r = its index in the grid, + stride, + 2 stride ... below n_docs, in that order: work(r, a, L, c0, c1) for the read
// text[a .. a + L) with c0, c1 its symbols lane and 64 + lane as read_load gives them.  SECOND: a second byte stream over the same
// offsets (the qualities) is prefetched alike, and the call is work(r, a, L, c0, c1, q0, q1).  Everything but the c and q is wave-uniform.
// The wave runs two reads ahead: while read r is worked on, the first 128 symbols of read r + stride and the offsets of read r + 2 stride
// are on their way, so a read of up to 128 symbols waits for no load of its own and the two dependent loads of a read (its offsets, then
// its bytes) overlap its neighbours'.  At the top of a trip (a1, L1) are the bounds of read r, whose first two words are asked for there,
// and (a0, L0, c0, c1) is read r - stride with those words, asked for a trip earlier; the bounds of read r + stride are asked for too, and
// waited for at the trip's end, behind the work on read r - stride.  No vector load is pending where a trip begins, so the wait for one
// trip's bytes is not a wait for the next trip's.  The last trip (more == false) asks for nothing and works on the wave's last read
template <bool SECOND, typename Work>
__device__ __forceinline__ void walk_reads(const uint8_t *text, const uint8_t *second, const uint64_t *doc_off, uint32_t n_docs, Work work)
{
    const uint32_t lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * RD_WAVES;
    uint64_t r = (uint64_t)blockIdx.x * RD_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t a0 = 0u, L0 = 0u, a1 = 0u, L1 = 0u;
    uint32_t c0 = 0u, c1 = 0u, q0 = 0u, q1 = 0u;
    if (r < n_docs) { a1 = uniform64(doc_off[r]); L1 = uniform64(doc_off[r + 1]) - a1; }
    for (bool first = true;; first = false, r += stride) {
        const bool more = r < n_docs;                                      // (L1 is 0 behind the last read: nothing is loaded)
        const uint32_t n0 = read_load(text + a1, L1, lane), n1 = read_load(text + a1, L1, 64u + lane);
        uint32_t m0 = 0u, m1 = 0u;
        if (SECOND) { m0 = read_load(second + a1, L1, lane); m1 = read_load(second + a1, L1, 64u + lane); }
        uint64_t a2 = 0u, L2 = 0u;
        if (r + stride < n_docs) { a2 = doc_off[r + stride]; L2 = doc_off[r + stride + 1]; }
        if (!first) {
            if constexpr (SECOND) work(r - stride, a0, L0, c0, c1, q0, q1);
            else work(r - stride, a0, L0, c0, c1);
        }
        if (!more) break;
        a0 = a1; L0 = L1; c0 = n0; c1 = n1; q0 = m0; q1 = m1;
        a1 = uniform64(a2); L1 = uniform64(L2) - a1;
    }
}

} // namespace lime
