// lime_adapter_kernel.hip -- where a 3' adapter begins in every read (include/lime_hip.h states the rule at lime_adapter_trim, the oracle;
// lime_docs.cpp sequences the passes: this kernel, the prefix sum over the new lengths and lime_fqtrim_kernel.hip's k_trim_copy).
//   k_adapter_bounds  per read lo32[r] = 0 and len32[r] = p*, the smallest start p in [0, L) at which the adapter, or the part of it
//                     that fits in front of the read's end, lies with few enough mismatches (L without one).  One wave on a read, 64
//                     symbols a step.  Lane i loads symbol 64 w + i where it lies in the read; four ballots of (byte & 0xDF) == b give
//                     the words R_b[w], b in A C G T, with 0 bits behind the read's end.  The adapter is four such words A_b, kernel
//                     arguments.  Lane p's window, bits p .. p + 63 of R_b, is the funnel shift of (R_b[w], R_b[w + 1]); the symbols
//                     that agree are the set bits of window_b & A_b summed over b: behind the read's end R_b holds no bit and behind
//                     the adapter's end A_b holds none, so the sum counts the k = min(M, L - p) overlapping places alone.  A ballot of
//                     "hit" and its lowest bit are the word's leftmost hit, and the wave leaves the read at the first word with one.
//                     A step holds the current word and the next and loads the one after: every byte is loaded once.
//                     A wave strides over its reads and runs two ahead (walk_reads, lime_reads.h): a read of up to 128 symbols waits
//                     for no load of its own.
// wave64.  The loops over the reads and over a read's words are wave-uniform (blockIdx, the wave's index and the read's length made
// scalar), and every ballot sits in them with the lanes outside the read taking part with no value.  No inline assembly, plain vector
// stores, no LDS.  No byte outside text[doc_off[r] .. doc_off[r + 1]) is loaded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_reads.h"

namespace lime {

namespace {

// p* of the read s[0 .. L): c0, c1 its symbols lane and 64 + lane as read_load gives them.  Every argument but c0, c1 is wave-uniform
__device__ __forceinline__ uint64_t ad_find(const uint8_t *s, uint64_t L, uint32_t c0, uint32_t c1, const uint64_t A[4], uint32_t M, uint32_t O, uint32_t E)
{
    const uint32_t lane = lane_id();
    const uint64_t n_words = (L + 63u) >> 6;
    BaseWords cur = base_words(c0), nxt = base_words(c1);
    for (uint64_t w = 0; w < n_words; ++w) {
        const uint32_t c2 = read_load(s, L, (w + 2u) * 64u + lane);        // (on its way while this word is worked on)
        const uint64_t p = w * 64u + lane;
        const uint64_t rest = p < L ? L - p : 0u;
        const uint32_t k = rest < M ? (uint32_t)rest : M;                  // the places at which read and adapter overlap
        uint32_t same = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint64_t win = (cur.b[b] >> lane) | ((nxt.b[b] << 1) << (63u - lane));
            same += (uint32_t)__builtin_popcountll(win & A[b]);
        }
        const bool hit = k >= O && k - same <= (k * E) / 100u;             // (O >= 1: a lane behind the read is no hit)
        const uint64_t hits = __ballot(hit);
        if (hits) return w * 64u + (uint32_t)__builtin_ctzll(hits);
        cur = nxt;
        nxt = base_words(c2);
    }
    return L;
}

// lo32[r], len32[r] of every read (len32[n_docs] stays as the caller zeroed it); counts[0] += reads that changed, counts[1] += reads with
// symbols that keep none.  A0 .. A3: bit j set where the adapter's symbol j is A, C, G, T.  1 <= O <= M <= 64, E <= 50
__global__ void __launch_bounds__(RD_WG) k_adapter_bounds(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, uint64_t A0, uint64_t A1, uint64_t A2,
                                                          uint64_t A3, uint32_t M, uint32_t O, uint32_t E, uint32_t *lo32, uint32_t *len32,
                                                          unsigned long long *counts)
{
    const uint32_t lane = lane_id();
    const uint64_t A[4] = {A0, A1, A2, A3};
    uint32_t changed = 0u, emptied = 0u;
    walk_reads<false>(text, nullptr, doc_off, n_docs, [&](uint64_t r, uint64_t a, uint64_t L, uint32_t c0, uint32_t c1) {
        const uint64_t keep = ad_find(text + a, L, c0, c1, A, M, O, E);
        if (lane == 0u) { lo32[r] = 0u; len32[r] = (uint32_t)keep; }       // (a read holds fewer than 2^32 symbols)
        changed += (uint32_t)(keep != L);
        emptied += (uint32_t)(L != 0u && keep == 0u);
    });
    if (lane == 0u) {
        if (changed) atomicAdd(&counts[0], (unsigned long long)changed);
        if (emptied) atomicAdd(&counts[1], (unsigned long long)emptied);
    }
}

} // namespace

void ad_launch_bounds(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const uint64_t masks[4], uint32_t m, uint32_t min_overlap,
                      uint32_t max_err_pct, uint32_t *lo32, uint32_t *len32, uint64_t *counts, hipStream_t st)
{
    const uint32_t grid = rd_grid(n_docs);
    if (grid)
        k_adapter_bounds<<<grid, RD_WG, 0, st>>>(text, doc_off, n_docs, masks[0], masks[1], masks[2], masks[3], m, min_overlap, max_err_pct, lo32, len32,
                                                 (unsigned long long *)counts);
}

} // namespace lime
