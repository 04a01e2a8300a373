// lime_filter_kernel.hip -- what the read filter keeps of every read (include/lime_hip.h states the rule at lime_read_filter, the oracle;
// lime_docs.cpp sequences the passes: this kernel, the prefix sum over the new lengths and lime_fqtrim_kernel.hip's k_trim_copy).
//   k_filter_bounds  per read lo32[r] = 0 and len32[r] = n, what the poly-X tail and the cap leave of it, or 0 where a filter fails it.
//                    One wave on a read, 64 symbols a word, in lime_reads.h's conventions: lane i loads symbol 64 w + i where it lies in
//                    the read, and base_words gives the words R_b[w], b in A C G T, with 0 bits behind the read's end; the fifth class
//                    "other" is what is valid and in none of them.
//                    The tail: the words from the last one down.  For a base X of the mask, lane j's mm_X is the set bits of
//                    ~R_X & valid at and above bit j plus the misses carried from the words behind; a lane is admissible when its
//                    symbol is X, its tail holds T symbols or more and 8 mm_X <= t.  A ballot of "admissible" (over every X of the mask)
//                    and its lowest bit are the word's longest tail; a lower word's replaces it.  X leaves the walk at the first word
//                    boundary with 8 carry_X > L (mm only grows, t <= L: no longer tail of X is admissible), and the walk ends where
//                    every X has left.
//                    The counts below n = min(L - t*, K): the N's by the set bits of "other", the equal neighbours by those of
//                    OR_b (R_b & (R_b >> 1 | the next word's bit 0 << 63)) over the five classes under the mask of the places
//                    j < n - 1, so that the pair across a word boundary counts once and the pair (n - 1, n) does not.  Ballots are
//                    wave-uniform: this pass is scalar work but for the loads.
//                    A read of up to 128 symbols is loaded once and its two words serve both passes; a longer one's tail walk loads
//                    from the end and its forward pass loads again, one word ahead each.
//                    A wave strides over its reads and runs two ahead (walk_reads, lime_reads.h).
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

struct FlArgs { uint32_t polyx_mask, polyx_min, max_len, min_len, max_n, min_complexity; };

// word w of the read: c0, c1 where they hold it, a load of its own otherwise (w is wave-uniform)
__device__ __forceinline__ uint32_t fl_fetch(const uint8_t *s, uint64_t L, uint64_t w, uint32_t c0, uint32_t c1, uint32_t lane)
{
    if (w == 0u) return c0;
    if (w == 1u) return c1;
    return read_load(s, L, w * 64u + lane);
}

// t* of the read s[0 .. L), L >= 1: the longest admissible tail over the bases of `mask`, 0 without one.  Wave-uniform but for c0, c1
__device__ __forceinline__ uint64_t fl_tail(const uint8_t *s, uint64_t L, uint32_t c0, uint32_t c1, uint32_t mask, uint32_t T)
{
    const uint32_t lane = lane_id();
    const uint64_t n_words = (L + 63u) >> 6;
    uint64_t carry[4] = {0u, 0u, 0u, 0u};
    uint32_t live = mask;                                                  // the bases that may still have a longer tail
    uint64_t best = L;                                                     // the smallest admissible start so far
    uint32_t nxt = fl_fetch(s, L, n_words - 1u, c0, c1, lane);
    for (uint64_t w = n_words; w-- > 0u && live;) {
        const uint32_t cur = nxt;
        if (w) nxt = fl_fetch(s, L, w - 1u, c0, c1, lane);                 // (on its way while this word is worked on)
        const BaseWords R = base_words(cur);
        const uint64_t valid = low_bits(L - w * 64u);
        const uint64_t p = w * 64u + lane;
        const uint64_t t = p < L ? L - p : 0u;                             // (a lane behind the read: t = 0 < T)
        bool adm = false;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (!(live >> b & 1u)) continue;
            const uint64_t miss = ~R.b[b] & valid;
            const uint64_t mm = (uint64_t)__builtin_popcountll(miss >> lane) + carry[b];
            adm = adm || ((R.b[b] >> lane & 1u) && t >= T && 8u * mm <= t);
            carry[b] += (uint64_t)__builtin_popcountll(miss);
            if (8u * carry[b] > L) live &= ~(1u << b);
        }
        const uint64_t hits = __ballot(adm);
        if (hits) best = w * 64u + (uint32_t)__builtin_ctzll(hits);
    }
    return L - best;
}

// of s[0 .. n), n >= 1 and n <= L: *n_other = its symbols that are no base, *n_equal = the j in [0, n - 1) whose symbol's class is that of
// the next.  Wave-uniform but for c0, c1
__device__ __forceinline__ void fl_counts(const uint8_t *s, uint64_t L, uint64_t n, uint32_t c0, uint32_t c1, uint64_t *n_other, uint64_t *n_equal)
{
    const uint32_t lane = lane_id();
    const uint64_t n_words = (n + 63u) >> 6;
    BaseWords cur = base_words(c0), nxt = base_words(c1);
    uint64_t other = 0u, equal = 0u;
    for (uint64_t w = 0; w < n_words; ++w) {
        uint32_t c2 = 0u;
        if (w + 2u < n_words) c2 = read_load(s, L, (w + 2u) * 64u + lane);   // (on its way while this word is worked on; a word the counts need)
        const uint64_t o_cur = ~(cur.b[0] | cur.b[1] | cur.b[2] | cur.b[3]), o_nxt = ~(nxt.b[0] | nxt.b[1] | nxt.b[2] | nxt.b[3]);
        const uint64_t below = n - w * 64u;                                // the places of this word in front of n, 1 and more
        other += (uint64_t)__builtin_popcountll(o_cur & low_bits(below));
        uint64_t eq = o_cur & ((o_cur >> 1) | (o_nxt << 63));
#pragma unroll
        for (int b = 0; b < 4; ++b) eq |= cur.b[b] & ((cur.b[b] >> 1) | (nxt.b[b] << 63));
        equal += (uint64_t)__builtin_popcountll(eq & low_bits(below - 1u));  // the pairs j, j + 1 with j + 1 < n
        cur = nxt;
        nxt = base_words(c2);
    }
    *n_other = other; *n_equal = equal;
}

// lo32[r], len32[r] of every read (len32[n_docs] stays as the caller zeroed it); counts[0 .. 5) += the reads with a poly-X tail, the reads
// the cap shortened, and the reads emptied as short, for their N's and for their complexity
__global__ void __launch_bounds__(RD_WG) k_filter_bounds(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, FlArgs f, uint32_t *lo32, uint32_t *len32,
                                                         unsigned long long *counts)
{
    const uint32_t lane = lane_id();
    uint32_t n_polyx = 0u, n_capped = 0u, n_short = 0u, n_many = 0u, n_low = 0u;
    const bool count = f.max_n != LIME_FILTER_OFF || f.min_complexity != 0u;
    walk_reads<false>(text, nullptr, doc_off, n_docs, [&](uint64_t r, uint64_t a, uint64_t L, uint32_t c0, uint32_t c1) {
        uint64_t keep = 0u;
        if (L) {                                                           // (a read that came in empty is counted nowhere)
            uint64_t n = L;
            if (f.polyx_mask) {
                const uint64_t t = fl_tail(text + a, L, c0, c1, f.polyx_mask, f.polyx_min);
                n_polyx += (uint32_t)(t != 0u);
                n -= t;
            }
            if (f.max_len && n > f.max_len) { n = f.max_len; ++n_capped; }
            // this read's share of three counts, added behind the branches: increments of the captured counters in branches that exclude
            // one another are merged into one increment through a chosen address, and the counters then live in scratch
            uint32_t d_short = 0u, d_many = 0u, d_low = 0u;
            bool pass = true;
            if (n < f.min_len) { pass = false; ++d_short; }
            else if (count && n) {
                uint64_t other, equal;
                fl_counts(text + a, L, n, c0, c1, &other, &equal);
                const uint64_t d = n - 1u - equal;
                if (f.max_n != LIME_FILTER_OFF && other > f.max_n) { pass = false; ++d_many; }
                else if (n >= 2u && 100u * d < (uint64_t)f.min_complexity * (n - 1u)) { pass = false; ++d_low; }
            }
            n_short += d_short; n_many += d_many; n_low += d_low;
            keep = pass ? n : 0u;
        }
        if (lane == 0u) { lo32[r] = 0u; len32[r] = (uint32_t)keep; }       // (a read holds fewer than 2^32 symbols)
    });
    if (lane == 0u) {
        if (n_polyx) atomicAdd(&counts[0], (unsigned long long)n_polyx);
        if (n_capped) atomicAdd(&counts[1], (unsigned long long)n_capped);
        if (n_short) atomicAdd(&counts[2], (unsigned long long)n_short);
        if (n_many) atomicAdd(&counts[3], (unsigned long long)n_many);
        if (n_low) atomicAdd(&counts[4], (unsigned long long)n_low);
    }
}

} // namespace

void fl_launch_bounds(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const lime_filter_t *f, uint32_t *lo32, uint32_t *len32, uint64_t *counts,
                      hipStream_t st)
{
    const uint32_t grid = rd_grid(n_docs);
    const FlArgs a = {f->polyx_mask, f->polyx_min, f->max_len, f->min_len, f->max_n, f->min_complexity};
    if (grid) k_filter_bounds<<<grid, RD_WG, 0, st>>>(text, doc_off, n_docs, a, lo32, len32, (unsigned long long *)counts);
}

} // namespace lime
