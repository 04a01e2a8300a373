// lime_qc_kernel.hip -- per-position statistics of the reads (include/lime_hip.h states the rule at lime_read_qc, the oracle; lime_docs.cpp
// sequences the call: the tables cleared, this kernel, the copy back).
//   k_qc_reads  tables += the counts of every read.  One wave on a read, 64 symbols a word, in k_filter_bounds' conventions: lane i of word
//               w loads symbol and quality byte 64 w + i where they lie in the read.
//               Rows p < n_pos: a per-workgroup table in LDS of 32-bit counters, counter-major ([counter][p], a counter's row P64 = n_pos
//               rounded up to 64 words long), behind it the three per-read histograms in the tables' order.  A lane with p < min(L, n_pos)
//               adds 1 to [class][p], its quality byte to [5][p] and 1 to [6][p], [7][p] where the byte reaches 53, 63 (ds_add_u32).  An LDS
//               add's bank is (address / 4) % 32 within a half-wave of 32 lanes; the lanes of a half hold 32 consecutive p and every counter's
//               row starts at a multiple of 64 words, so whatever their classes the 32 lanes fall on 32 different banks: no conflict by the
//               rule (SQ_LDS_BANK_CONFLICT was not taken).
//               Row n_pos (the pool) and the per-read sums are wave-uniform work.  Four ballots of (byte & 0xDF) == b give R_b, with 0
//               bits behind the read's end; "other" is what is valid and in none.  Under the mask of the lanes with p >= n_pos their set bits
//               are the pool's class counts; over the whole word those of R_C | R_G and of the four are the read's gc and acgt.  Eight ballots
//               of the quality byte's bits give the sums without a cross-lane reduction (the sum of popcount(bit k's ballot) << k), under the
//               pool's mask and over the word; two ballots of byte >= 53, >= 63 give the pool's q20, q30.  The pool's eight counters are
//               64-bit words in LDS, in front of the table: lane k < 8 of a word with pooled lanes adds the word's count k (at most 64 * 255)
//               to counter k (ds_add_u64), so that no wave carries sixteen scalar registers over its reads.
//               The per-read histograms: lane 0 adds 1 in LDS at min(L, n_pos), at (100 gc) / acgt where acgt >= 1, at qsum / L where L >= 1
//               and there are qualities: one add each per read.
//               Flush: once per workgroup, behind a barrier, its non-zero LDS counters are added to the 64-bit tables (atomicAdd on
//               unsigned long long): integers, so the result does not depend on the order.
//               A wave strides over its reads and runs two ahead, as k_filter_bounds does: the first 128 symbols (and quality bytes) of read
//               r + stride and the offsets of read r + 2 stride are on their way while read r is worked on; within a read the word after the
//               next is.
// Why the 32-bit counters of the rows p < n_pos cannot overflow: a read adds at most 1 to a class, q20 or q30 counter of a row and at most
// 255 to its qsum, and 1 to one counter of each histogram.  A workgroup handles QC_WAVES reads per trip and ceil(n_docs / (QC_WAVES * grid))
// trips; the grid is min(ceil(n_docs / QC_WAVES), QC_BLOCKS), so with n_docs <= 2^32 - 1 a workgroup sees at most QC_WAVES * 2^32 /
// (QC_WAVES * QC_BLOCKS) = 2^21 reads, and no counter passes 255 * 2^21 < 2^29.  Only the pool can: one long read pushes its qsum past 2^32
// at 16.9 million symbols; it and the per-read sums (100 gc of a read that is the whole text) are 64 bits wide.
// wave64.  The loops over the reads and over a read's words are wave-uniform (blockIdx, the wave's index and the read's length made scalar),
// and every ballot sits in them with the lanes outside the read taking part with no value.  No inline assembly, plain vector stores and
// vector atomics only.  No byte outside text[doc_off[r] .. doc_off[r + 1]) is loaded, and likewise for qual.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_wave.h"

namespace lime {

namespace {

constexpr int QC_WG = 256;
constexpr uint32_t QC_WAVES = QC_WG / 64;        // reads a workgroup handles per trip
constexpr uint32_t QC_BLOCKS = 2048;             // eight workgroups a CU (19.5 KB of LDS each at most, 160 KB a CU): the grid is capped and the waves stride

__device__ __forceinline__ uint64_t qc_uniform64(uint64_t v)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// byte `at` of the read s[0 .. L) as it is, 0 outside it
__device__ __forceinline__ uint32_t qc_load(const uint8_t *s, uint64_t L, uint64_t at)
{
    return at < L ? (uint32_t)s[at] : 0u;
}

// the k lowest bits, k in 0 .. 64 and above
__device__ __forceinline__ uint64_t qc_low(uint64_t k)
{
    return k >= 64u ? ~0ull : (1ull << k) - 1u;
}

__device__ __forceinline__ uint64_t qc_pop(uint64_t m) { return (uint64_t)__builtin_popcountll(m); }

// QUAL: the documents carry qualities (qual is not NULL)
template <bool QUAL>
__global__ void __launch_bounds__(QC_WG) k_qc_reads(const uint8_t *text, const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t n_pos,
                                                    unsigned long long *tables)
{
    extern __shared__ unsigned long long pool[]; // the pool's eight counters, then the 32-bit table:
    uint32_t *const lds = reinterpret_cast<uint32_t *>(pool + 8);            // [8][P64] counters, len_hist[n_pos + 1], gc_hist[101], mq_hist[256]
    const uint32_t P64 = (n_pos + 63u) & ~63u;
    const uint32_t H = 8u * P64;                 // where the histograms begin
    const uint32_t n_hist = n_pos + 1u + 101u + 256u;
    for (uint32_t i = threadIdx.x; i < H + n_hist; i += QC_WG) lds[i] = 0u;
    if (threadIdx.x < 8u) pool[threadIdx.x] = 0ull;
    __syncthreads();

    const uint32_t lane = lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * QC_WAVES;
    uint64_t r = (uint64_t)blockIdx.x * QC_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // two reads ahead, as in k_filter_bounds: at the top of a trip (a1, L1) are the bounds of read r, whose first two words are asked for
    // there, and (a0, L0, c0, c1, q0, q1) is read r - stride with those words; the bounds of read r + stride are asked for too
    // (a text holds fewer than 2^32 symbols: a read's length, its words and its counts of symbols are 32 bits wide, its sums are not)
    uint64_t a0 = 0u, a1 = 0u;
    uint32_t L0 = 0u, L1 = 0u;
    uint32_t c0 = 0u, c1 = 0u, q0 = 0u, q1 = 0u;
    if (r < n_docs) { a1 = qc_uniform64(doc_off[r]); L1 = (uint32_t)(qc_uniform64(doc_off[r + 1]) - a1); }
    for (bool first = true;; first = false, r += stride) {
        const bool more = r < n_docs;                                      // (L1 is 0 behind the last read: nothing is loaded)
        const uint32_t n0 = qc_load(text + a1, L1, lane), n1 = qc_load(text + a1, L1, 64u + lane);
        uint32_t m0 = 0u, m1 = 0u;
        if (QUAL) { m0 = qc_load(qual + a1, L1, lane); m1 = qc_load(qual + a1, L1, 64u + lane); }
        uint64_t a2 = 0u, L2 = 0u;
        if (r + stride < n_docs) { a2 = doc_off[r + stride]; L2 = doc_off[r + stride + 1]; }
        if (!first) {
            const uint8_t *s = text + a0, *sq = qual + a0;
            const uint32_t n_words = (L0 >> 6) + ((L0 & 63u) != 0u);
            uint32_t gc = 0u, acgt = 0u;
            uint64_t qs = 0u;
            uint32_t cc = c0, cn = c1, qc = q0, qn = q1;
            for (uint32_t w = 0; w < n_words; ++w) {
                uint32_t c2 = 0u, q2 = 0u;
                if (w + 2u < n_words) {                                    // (on its way while this word is worked on)
                    c2 = qc_load(s, L0, ((uint64_t)w + 2u) * 64u + lane);
                    if (QUAL) q2 = qc_load(sq, L0, ((uint64_t)w + 2u) * 64u + lane);
                }
                const uint32_t base = w * 64u;                             // (below L0)
                const uint64_t valid = qc_low(L0 - base);
                const uint32_t c = cc & 0xDFu;                             // (lower case is its base)
                const uint64_t RA = __ballot(c == 'A'), RC = __ballot(c == 'C'), RG = __ballot(c == 'G'), RT = __ballot(c == 'T');
                const uint64_t any = RA | RC | RG | RT;
                gc += (uint32_t)qc_pop(RC | RG);
                acgt += (uint32_t)qc_pop(any);
                // the lanes of this word at and behind n_pos: the pool's
                const uint64_t pm = valid & ~qc_low(n_pos > base ? n_pos - base : 0u);
                uint32_t mine = 0u;                                        // lane k < 8: this word's count for the pool's counter k
                if (pm) {
                    mine = lane == 0u ? (uint32_t)qc_pop(RA & pm) : lane == 1u ? (uint32_t)qc_pop(RC & pm) : lane == 2u ? (uint32_t)qc_pop(RG & pm)
                         : lane == 3u ? (uint32_t)qc_pop(RT & pm) : lane == 4u ? (uint32_t)qc_pop(~any & pm) : 0u;
                }
                if (QUAL) {
                    uint64_t sum = 0u, psum = 0u;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const uint64_t bk = __ballot((qc >> k & 1u) != 0u);    // (a lane behind the read holds 0)
                        sum += qc_pop(bk) << k;
                        psum += qc_pop(bk & pm) << k;
                    }
                    qs += sum;
                    const uint64_t b20 = __ballot(qc >= 53u), b30 = __ballot(qc >= 63u);
                    if (pm) mine = lane == 5u ? (uint32_t)psum : lane == 6u ? (uint32_t)qc_pop(b20 & pm) : lane == 7u ? (uint32_t)qc_pop(b30 & pm) : mine;
                }
                if (pm && lane < 8u && mine) atomicAdd(&pool[lane], (unsigned long long)mine);
                if (base < n_pos) {                                        // the rows of their own: LDS adds, lanes with p < min(L, n_pos)
                    const uint32_t p = base + lane;
                    if (p < n_pos && p < L0) {
                        const uint32_t cls = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
                        atomicAdd(&lds[cls * P64 + p], 1u);
                        if (QUAL) {
                            atomicAdd(&lds[5u * P64 + p], qc);
                            if (qc >= 53u) atomicAdd(&lds[6u * P64 + p], 1u);
                            if (qc >= 63u) atomicAdd(&lds[7u * P64 + p], 1u);
                        }
                    }
                }
                cc = cn; cn = c2; qc = qn; qn = q2;
            }
            if (lane == 0u) {                                              // one add per read and histogram
                atomicAdd(&lds[H + (L0 < n_pos ? L0 : n_pos)], 1u);
                if (acgt) atomicAdd(&lds[H + n_pos + 1u + (uint32_t)(100ull * gc / acgt)], 1u);
                if (QUAL && L0) atomicAdd(&lds[H + n_pos + 1u + 101u + (uint32_t)(qs / L0)], 1u);
            }
        }
        if (!more) break;
        a0 = a1; L0 = L1; c0 = n0; c1 = n1; q0 = m0; q1 = m1;
        a1 = qc_uniform64(a2); L1 = (uint32_t)(qc_uniform64(L2) - a1);
    }
    __syncthreads();
    if (threadIdx.x < 8u && pool[threadIdx.x]) atomicAdd(&tables[8u * n_pos + threadIdx.x], pool[threadIdx.x]);
    for (uint32_t i = threadIdx.x; i < H + n_hist; i += QC_WG) {
        const uint32_t v = lds[i];
        if (!v) continue;
        if (i < H) {
            const uint32_t k = i / P64, p = i - k * P64;                   // (the pad behind n_pos stays 0)
            atomicAdd(&tables[8u * p + k], (unsigned long long)v);
        } else {
            atomicAdd(&tables[8u * (n_pos + 1u) + (i - H)], (unsigned long long)v);
        }
    }
}

} // namespace

void qc_launch_reads(const uint8_t *text, const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t n_pos, uint64_t *tables, hipStream_t st)
{
    const uint64_t nb = ((uint64_t)n_docs + QC_WAVES - 1u) / QC_WAVES;
    if (!nb) return;
    const uint32_t grid = nb < QC_BLOCKS ? (uint32_t)nb : QC_BLOCKS;
    const uint32_t P64 = (n_pos + 63u) & ~63u;
    const size_t lds_bytes = 64u + (8u * (size_t)P64 + n_pos + 1u + 101u + 256u) * 4u;
    if (qual) k_qc_reads<true><<<grid, QC_WG, lds_bytes, st>>>(text, qual, doc_off, n_docs, n_pos, (unsigned long long *)tables);
    else k_qc_reads<false><<<grid, QC_WG, lds_bytes, st>>>(text, nullptr, doc_off, n_docs, n_pos, (unsigned long long *)tables);
}

} // namespace lime
