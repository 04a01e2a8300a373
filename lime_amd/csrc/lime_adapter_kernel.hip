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
//                     A wave strides over its reads and runs two ahead: while read r is worked on, the first 128 symbols of read
//                     r + stride and the offsets of read r + 2 stride are on their way, so a read of up to 128 symbols waits for no
//                     load of its own and the two dependent loads of a read (its offsets, then its bytes) overlap its neighbours'.
// wave64.  The loops over the reads and over a read's words are wave-uniform (blockIdx, the wave's index and the read's length made
// scalar), and every ballot sits in them with the lanes outside the read taking part with no value.  No inline assembly, plain vector
// stores, no LDS.  No byte outside text[doc_off[r] .. doc_off[r + 1]) is loaded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_wave.h"

namespace lime {

namespace {

constexpr int AD_WG = 256;
constexpr uint32_t AD_WAVES = AD_WG / 64;        // reads a workgroup handles per trip
constexpr uint32_t AD_BLOCKS = 2048;             // eight workgroups a CU: the grid is capped and the waves stride

struct AdWords { uint64_t b[4]; };               // R_A, R_C, R_G, R_T of 64 symbols

__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// symbol `at` of the read s[0 .. L) as it is, 0 (no base) outside it.  Nothing is done to the byte here: a prefetched one is waited for
// where ad_words folds it, not where it is asked for
__device__ __forceinline__ uint32_t ad_load(const uint8_t *s, uint64_t L, uint64_t at)
{
    return at < L ? (uint32_t)s[at] : 0u;
}

__device__ __forceinline__ AdWords ad_words(uint32_t c)
{
    AdWords w;
    c &= 0xDFu;                                  // (lower case matches)
    w.b[0] = __ballot(c == 'A'); w.b[1] = __ballot(c == 'C'); w.b[2] = __ballot(c == 'G'); w.b[3] = __ballot(c == 'T');
    return w;
}

// p* of the read s[0 .. L): c0, c1 its symbols lane and 64 + lane as ad_load gives them.  Every argument but c0, c1 is wave-uniform
__device__ __forceinline__ uint64_t ad_find(const uint8_t *s, uint64_t L, uint32_t c0, uint32_t c1, const uint64_t A[4], uint32_t M, uint32_t O, uint32_t E)
{
    const uint32_t lane = lane_id();
    const uint64_t n_words = (L + 63u) >> 6;
    AdWords cur = ad_words(c0), nxt = ad_words(c1);
    for (uint64_t w = 0; w < n_words; ++w) {
        const uint32_t c2 = ad_load(s, L, (w + 2u) * 64u + lane);          // (on its way while this word is worked on)
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
        nxt = ad_words(c2);
    }
    return L;
}

// lo32[r], len32[r] of every read (len32[n_docs] stays as the caller zeroed it); counts[0] += reads that changed, counts[1] += reads with
// symbols that keep none.  A0 .. A3: bit j set where the adapter's symbol j is A, C, G, T.  1 <= O <= M <= 64, E <= 50
__global__ void __launch_bounds__(AD_WG) k_adapter_bounds(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, uint64_t A0, uint64_t A1, uint64_t A2,
                                                          uint64_t A3, uint32_t M, uint32_t O, uint32_t E, uint32_t *lo32, uint32_t *len32,
                                                          unsigned long long *counts)
{
    const uint32_t lane = lane_id();
    const uint64_t A[4] = {A0, A1, A2, A3};
    const uint64_t stride = (uint64_t)gridDim.x * AD_WAVES;
    uint64_t r = (uint64_t)blockIdx.x * AD_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // The wave runs two reads ahead.  At the top of a trip (a1, L1) are the bounds of read r, whose first two words are asked for there, and
    // (a0, L0, c0, c1) is read r - stride with those words, asked for a trip earlier; the bounds of read r + stride are asked for too, and
    // waited for at the trip's end, behind the work on read r - stride.  No vector load is pending where a trip begins, so the wait for one
    // trip's bytes is not a wait for the next trip's
    uint64_t a0 = 0u, L0 = 0u, a1 = 0u, L1 = 0u;
    uint32_t c0 = 0u, c1 = 0u;
    if (r < n_docs) { a1 = uniform64(doc_off[r]); L1 = uniform64(doc_off[r + 1]) - a1; }
    uint32_t changed = 0u, emptied = 0u;
    for (bool first = true;; first = false, r += stride) {
        const bool more = r < n_docs;                                      // (L1 is 0 behind the last read: nothing is loaded)
        const uint32_t n0 = ad_load(text + a1, L1, lane), n1 = ad_load(text + a1, L1, 64u + lane);
        uint64_t a2 = 0u, L2 = 0u;
        if (r + stride < n_docs) { a2 = doc_off[r + stride]; L2 = doc_off[r + stride + 1]; }
        if (!first) {
            const uint64_t keep = ad_find(text + a0, L0, c0, c1, A, M, O, E);
            if (lane == 0u) { lo32[r - stride] = 0u; len32[r - stride] = (uint32_t)keep; }      // (a read holds fewer than 2^32 symbols)
            changed += (uint32_t)(keep != L0);
            emptied += (uint32_t)(L0 != 0u && keep == 0u);
        }
        if (!more) break;
        a0 = a1; L0 = L1; c0 = n0; c1 = n1;
        a1 = uniform64(a2); L1 = uniform64(L2) - a1;
    }
    if (lane == 0u) {
        if (changed) atomicAdd(&counts[0], (unsigned long long)changed);
        if (emptied) atomicAdd(&counts[1], (unsigned long long)emptied);
    }
}

} // namespace

void ad_launch_bounds(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const uint64_t masks[4], uint32_t m, uint32_t min_overlap,
                      uint32_t max_err_pct, uint32_t *lo32, uint32_t *len32, uint64_t *counts, hipStream_t st)
{
    const uint64_t nb = ((uint64_t)n_docs + AD_WAVES - 1u) / AD_WAVES;
    if (nb)
        k_adapter_bounds<<<nb < AD_BLOCKS ? (uint32_t)nb : AD_BLOCKS, AD_WG, 0, st>>>(text, doc_off, n_docs, masks[0], masks[1], masks[2], masks[3], m, min_overlap,
                                                                           max_err_pct, lo32, len32, (unsigned long long *)counts);
}

} // namespace lime
