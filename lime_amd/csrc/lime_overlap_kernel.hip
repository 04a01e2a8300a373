// lime_overlap_kernel.hip -- where the two mates of a pair run through their fragment into the adapter, found from the mates' overlap alone
// (include/lime_hip.h states the rule at lime_pair_overlap_trim, the oracle; lime_docs.cpp sequences the passes: this kernel, then per mate
// the prefix sum over the new lengths and lime_fqtrim_kernel.hip's k_trim_copy).  lime_reads.h's conventions in their two-sequence form.
//   k_overlap_bounds  per pair r the insert I*, the largest admissible I in [O, La + Lb - O]; len1[r] = min(La, I*), len2[r] = min(Lb, I*)
//                     (the lengths as they are without one), lo1[r] = lo2[r] = 0, insert32[r] = I* or 0.  One wave on a pair.
//                     Mate 1 is a[0 .. La): lane i of word w loads a[64 w + i] where it lies in the read, and four ballots of
//                     (byte & 0xDF) == c give the words A_c[w], c in A C G T, with 0 bits behind the read's end.  Mate 2 enters as its
//                     reverse complement B'[k] = comp(b[Lb - 1 - k]) without being reversed anywhere: lane i of word w loads
//                     b[Lb - 1 - (64 w + i)] and the ballots are taken on the complement's class (a T sets the A word's bit, a G the C
//                     word's, ...).  A byte that is no base sets no bit in either read, so it agrees with nothing.
//                     Place j of candidate I compares a[j] with B'[j + d], d = Lb - I: a candidate is a shift d of B' against A, and the
//                     agreeing places are the set bits of A_c[w] & (bits 64 w + d .. 64 w + d + 63 of B'_c) summed over c and w.  Behind
//                     either read's end the words hold no bit, so only the n(I) places count; n(I) itself is arithmetic.
//                     A lane takes one candidate: step k holds the shifts d = 64 k + lane, so a lane's window of B' is the funnel shift
//                     by `lane` of the word pair (B'_c[w + k], B'_c[w + k + 1]), whose indices are the same in every lane.  The steps run
//                     from k = floor((O - La) / 64) up, that is from the largest I down (the first step's lanes below O - La and the last
//                     step's above Lb - O are no candidates); a ballot of "admissible" and its lowest bit are the step's largest I, and the
//                     wave leaves the pair at the first step with a hit.  Within a step only the w with a word of B' under the window are
//                     visited, and B'[w + k + 1] is the next w's B'[w + k].
//                     The words of the first OV_CAP * 64 = 512 symbols of each mate are made once per pair and kept in LDS (32 bytes a
//                     word of four classes, read back at one address by every lane); words beyond are made again from the text, which
//                     the caches hold, every time they are wanted: reads of any length and La != Lb are taken, at a cost that is
//                     quadratic in the length.
//                     A wave strides over its pairs and runs two ahead, as walk_reads does with reads: while pair r is worked on, the
//                     first word of both mates of pair r + stride and the four offsets of pair r + 2 stride are on their way.
// wave64.  The loops over the pairs, the steps and the words are wave-uniform (blockIdx, the wave's index and the lengths made scalar), and
// every ballot sits in them with the lanes outside a read taking part with no value.  No inline assembly, plain vector stores; LDS is
// written by every lane with the wave's one value and read by the same wave only: no barrier.  No byte outside
// text1[doc_off1[r] .. doc_off1[r + 1]) and text2[doc_off2[r] .. doc_off2[r + 1]) is loaded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_reads.h"

namespace lime {

namespace {

constexpr uint32_t OV_CAP = 8;                   // words of a mate kept in LDS: 512 symbols

// symbol `at` of mate 2 read backwards, b[L - 1 - at] of b[0 .. L), as it is; 0 outside it (mate 1 goes through read_load)
__device__ __forceinline__ uint32_t ov_load_rev(const uint8_t *b, uint64_t L, uint64_t at)
{
    return at < L ? (uint32_t)b[L - 1u - at] : 0u;
}

__device__ __forceinline__ BaseWords ov_words_comp(uint32_t c)    // base_words of the complement's class
{
    BaseWords w;
    c &= 0xDFu;
    w.b[0] = __ballot(c == 'T'); w.b[1] = __ballot(c == 'G'); w.b[2] = __ballot(c == 'C'); w.b[3] = __ballot(c == 'A');
    return w;
}

__device__ __forceinline__ void ov_keep(uint64_t *sm, uint32_t w, const BaseWords &x)       // (every lane writes the wave's one value)
{
#pragma unroll
    for (int b = 0; b < 4; ++b) sm[w * 4u + b] = x.b[b];
}

// word q of mate 1, 0 <= q < nA.  q is wave-uniform
__device__ __forceinline__ BaseWords ov_word_a(const uint64_t *sm, const uint8_t *a, uint64_t La, uint64_t q)
{
    BaseWords x;
    if (q < OV_CAP) {
#pragma unroll
        for (int b = 0; b < 4; ++b) x.b[b] = sm[q * 4u + b];
    } else {
        x = base_words(read_load(a, La, q * 64u + lane_id()));
    }
    return x;
}

// word q of mate 2's reverse complement; no bits for q outside [0, nB).  q is wave-uniform
__device__ __forceinline__ BaseWords ov_word_b(const uint64_t *sm, const uint8_t *b, uint64_t Lb, int64_t nB, int64_t q)
{
    BaseWords x;
    if (q < 0 || q >= nB) {
        x.b[0] = x.b[1] = x.b[2] = x.b[3] = 0u;
    } else if (q < (int64_t)OV_CAP) {
#pragma unroll
        for (int c = 0; c < 4; ++c) x.b[c] = sm[(uint64_t)q * 4u + c];
    } else {
        x = ov_words_comp(ov_load_rev(b, Lb, (uint64_t)q * 64u + lane_id()));
    }
    return x;
}

__device__ __forceinline__ int64_t floor_div64(int64_t v) { return v >> 6; }          // (an arithmetic shift: the floor, for negative v too)

// I* of the mates a[0 .. La), b[0 .. Lb), 0 without one: ca0, cb0 their symbols `lane` (b's read backwards) as read_load and ov_load_rev give them.  Every
// argument but ca0, cb0 is wave-uniform.  smA, smB: the wave's OV_CAP * 4 words each
__device__ __forceinline__ uint64_t ov_find(uint64_t *smA, uint64_t *smB, const uint8_t *a, uint64_t La, const uint8_t *b, uint64_t Lb, uint32_t ca0, uint32_t cb0,
                                            uint64_t O, uint64_t E)
{
    if (La + Lb < 2u * O || La == 0u || Lb == 0u) return 0u;              // (no candidate; an empty mate gives no overlap)
    const uint32_t lane = lane_id();
    const int64_t nA = (int64_t)((La + 63u) >> 6), nB = (int64_t)((Lb + 63u) >> 6);
    const int64_t keepA = nA < (int64_t)OV_CAP ? nA : (int64_t)OV_CAP, keepB = nB < (int64_t)OV_CAP ? nB : (int64_t)OV_CAP;
    ov_keep(smA, 0u, base_words(ca0));
    for (int64_t w = 1; w < keepA; ++w) ov_keep(smA, (uint32_t)w, base_words(read_load(a, La, (uint64_t)w * 64u + lane)));
    ov_keep(smB, 0u, ov_words_comp(cb0));
    for (int64_t w = 1; w < keepB; ++w) ov_keep(smB, (uint32_t)w, ov_words_comp(ov_load_rev(b, Lb, (uint64_t)w * 64u + lane)));
    const int64_t d_lo = (int64_t)O - (int64_t)La, d_hi = (int64_t)Lb - (int64_t)O;   // the shifts of the candidates I = La + Lb - O .. O
    for (int64_t k = floor_div64(d_lo); k <= floor_div64(d_hi); ++k) {
        const int64_t w0 = -k - 1 > 0 ? -k - 1 : 0, w1 = nB - k < nA ? nB - k : nA;    // the w with B'[w + k] or B'[w + k + 1] inside B'
        uint32_t same = 0u;
        BaseWords cur = ov_word_b(smB, b, Lb, nB, w0 + k);
        for (int64_t w = w0; w < w1; ++w) {
            const BaseWords nxt = ov_word_b(smB, b, Lb, nB, w + k + 1);
            const BaseWords x = ov_word_a(smA, a, La, (uint64_t)w);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint64_t win = (cur.b[c] >> lane) | ((nxt.b[c] << 1) << (63u - lane));
                same += (uint32_t)__builtin_popcountll(win & x.b[c]);
            }
            cur = nxt;
        }
        const int64_t d = k * 64 + (int64_t)lane;
        const bool cand = d >= d_lo && d <= d_hi;
        const uint64_t I = cand ? (uint64_t)((int64_t)Lb - d) : 0u;
        const uint64_t j0 = I > Lb ? I - Lb : 0u, j1 = La < I ? La : I;
        const uint64_t n = j1 > j0 ? j1 - j0 : 0u;
        const bool hit = cand && n >= O && n - same <= (n * E) / 100u;
        const uint64_t hits = __ballot(hit);
        if (hits) return (uint64_t)((int64_t)Lb - (k * 64 + (int64_t)__builtin_ctzll(hits)));        // (the lowest lane: the largest I)
    }
    return 0u;
}

// lo1, len1, lo2, len2 and insert32 (may be NULL) of every pair (len*[n_docs] stay as the caller zeroed them); counts[0] += pairs with an I*,
// counts[1] += pairs of which a mate got shorter.  O >= 1, E <= 50
__global__ void __launch_bounds__(RD_WG) k_overlap_bounds(const uint8_t *text1, const uint64_t *doc_off1, const uint8_t *text2, const uint64_t *doc_off2,
                                                          uint32_t n_docs, uint32_t O, uint32_t E, uint32_t *lo1, uint32_t *len1, uint32_t *lo2, uint32_t *len2,
                                                          uint32_t *insert32, unsigned long long *counts)
{
    __shared__ uint64_t sm[RD_WAVES][2][OV_CAP * 4u];
    const uint32_t lane = lane_id();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t stride = (uint64_t)gridDim.x * RD_WAVES;
    uint64_t r = (uint64_t)blockIdx.x * RD_WAVES + wave;
    // The wave runs two pairs ahead: walk_reads' trip (lime_reads.h) with a pair in a read's place.  It is written out here because a pair
    // has two texts and two offset arrays, one prefetched word a mate, and mate 2's loaded backwards: walk_reads would be a second walk
    // under a flag.  At the top of a trip (a1, La1, b1, Lb1) are the bounds of pair r, whose first words are asked for there, and
    // (a0, La0, b0, Lb0, ca, cb) is pair r - stride with those words, asked for a trip earlier; the bounds of pair r + stride are asked for
    // too, and waited for at the trip's end, behind the work on pair r - stride
    uint64_t a0 = 0u, La0 = 0u, b0 = 0u, Lb0 = 0u, a1 = 0u, La1 = 0u, b1 = 0u, Lb1 = 0u;
    uint32_t ca = 0u, cb = 0u;
    if (r < n_docs) {
        a1 = uniform64(doc_off1[r]); La1 = uniform64(doc_off1[r + 1]) - a1;
        b1 = uniform64(doc_off2[r]); Lb1 = uniform64(doc_off2[r + 1]) - b1;
    }
    uint32_t found = 0u, cut = 0u;
    for (bool first = true;; first = false, r += stride) {
        const bool more = r < n_docs;                                      // (La1 = Lb1 = 0 behind the last pair: nothing is loaded)
        const uint32_t na = read_load(text1 + a1, La1, lane), nb = ov_load_rev(text2 + b1, Lb1, lane);
        uint64_t a2 = 0u, a2e = 0u, b2 = 0u, b2e = 0u;
        if (r + stride < n_docs) { a2 = doc_off1[r + stride]; a2e = doc_off1[r + stride + 1]; b2 = doc_off2[r + stride]; b2e = doc_off2[r + stride + 1]; }
        if (!first) {
            const uint64_t I = ov_find(sm[wave][0], sm[wave][1], text1 + a0, La0, text2 + b0, Lb0, ca, cb, O, E);
            const uint64_t k1 = I && I < La0 ? I : La0, k2 = I && I < Lb0 ? I : Lb0;
            if (lane == 0u) {
                lo1[r - stride] = 0u; len1[r - stride] = (uint32_t)k1;     // (a read holds fewer than 2^32 symbols)
                lo2[r - stride] = 0u; len2[r - stride] = (uint32_t)k2;
                if (insert32) insert32[r - stride] = (uint32_t)I;
            }
            found += (uint32_t)(I != 0u);
            cut += (uint32_t)(k1 != La0 || k2 != Lb0);
        }
        if (!more) break;
        a0 = a1; La0 = La1; b0 = b1; Lb0 = Lb1; ca = na; cb = nb;
        a1 = uniform64(a2); La1 = uniform64(a2e) - a1;
        b1 = uniform64(b2); Lb1 = uniform64(b2e) - b1;
    }
    if (lane == 0u) {
        if (found) atomicAdd(&counts[0], (unsigned long long)found);
        if (cut) atomicAdd(&counts[1], (unsigned long long)cut);
    }
}

} // namespace

void ov_launch_bounds(const uint8_t *text1, const uint64_t *doc_off1, const uint8_t *text2, const uint64_t *doc_off2, uint32_t n_docs, uint32_t min_overlap,
                      uint32_t max_err_pct, uint32_t *lo1, uint32_t *len1, uint32_t *lo2, uint32_t *len2, uint32_t *insert32, uint64_t *counts, hipStream_t st)
{
    const uint32_t grid = rd_grid(n_docs);
    if (grid)
        k_overlap_bounds<<<grid, RD_WG, 0, st>>>(text1, doc_off1, text2, doc_off2, n_docs, min_overlap, max_err_pct, lo1, len1, lo2, len2, insert32,
                                                 (unsigned long long *)counts);
}

} // namespace lime
