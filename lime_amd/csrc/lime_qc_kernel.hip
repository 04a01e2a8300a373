// lime_qc_kernel.hip -- per-position statistics of the reads (include/lime_hip.h states the rule at lime_read_qc, the oracle; lime_docs.cpp
// sequences the call: the tables cleared, this kernel, the copy back).
//   k_qc_reads  tables += the counts of every read.  One wave on a read, 64 symbols a word, in lime_reads.h's conventions: lane i of word
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
//               A wave strides over its reads and runs two ahead (walk_reads, lime_reads.h, with the qualities as its second stream); within
//               a read the word after the next is on its way.
// Why the 32-bit counters of the rows p < n_pos cannot overflow: a read adds at most 1 to a class, q20 or q30 counter of a row and at most
// 255 to its qsum, and 1 to one counter of each histogram.  A workgroup handles RD_WAVES reads per trip and ceil(n_docs / (RD_WAVES * grid))
// trips; the grid is rd_grid(n_docs) = min(ceil(n_docs / RD_WAVES), RD_BLOCKS), so with n_docs <= 2^32 - 1 a workgroup sees at most
// RD_WAVES * 2^32 / (RD_WAVES * RD_BLOCKS) = 2^21 reads, and no counter passes 255 * 2^21 < 2^29 (the static_assert below).  Only the pool
// can: one long read pushes its qsum past 2^32 at 16.9 million symbols; it and the per-read sums (100 gc of a read that is the whole text)
// are 64 bits wide.  Eight workgroups a CU hold 19.5 KB of LDS each at most, of 160 KB.
// wave64.  The loops over the reads and over a read's words are wave-uniform (blockIdx, the wave's index and the read's length made scalar),
// and every ballot sits in them with the lanes outside the read taking part with no value.  No inline assembly, plain vector stores and
// vector atomics only.  No byte outside text[doc_off[r] .. doc_off[r + 1]) is loaded, and likewise for qual.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_reads.h"

namespace lime {

namespace {

// (what the argument above needs of the geometry: a workgroup sees at most 2^32 / RD_BLOCKS reads, each adding at most 255 to a counter)
static_assert(255ull * ((1ull << 32) / RD_BLOCKS) < (1ull << 32), "a 32-bit counter of k_qc_reads' LDS table could overflow");

__device__ __forceinline__ uint64_t qc_pop(uint64_t m) { return (uint64_t)__builtin_popcountll(m); }

// QUAL: the documents carry qualities (qual is not NULL)
template <bool QUAL>
__global__ void __launch_bounds__(RD_WG) k_qc_reads(const uint8_t *text, const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t n_pos,
                                                    unsigned long long *tables)
{
    extern __shared__ unsigned long long pool[]; // the pool's eight counters, then the 32-bit table:
    uint32_t *const lds = reinterpret_cast<uint32_t *>(pool + 8);            // [8][P64] counters, len_hist[n_pos + 1], gc_hist[101], mq_hist[256]
    const uint32_t P64 = (n_pos + 63u) & ~63u;
    const uint32_t H = 8u * P64;                 // where the histograms begin
    const uint32_t n_hist = n_pos + 1u + 101u + 256u;
    for (uint32_t i = threadIdx.x; i < H + n_hist; i += RD_WG) lds[i] = 0u;
    if (threadIdx.x < 8u) pool[threadIdx.x] = 0ull;
    __syncthreads();

    const uint32_t lane = lane_id();
    walk_reads<QUAL>(text, qual, doc_off, n_docs, [&](uint64_t, uint64_t a, uint64_t L, uint32_t c0, uint32_t c1, uint32_t q0 = 0u, uint32_t q1 = 0u) {
        // (a text holds fewer than 2^32 symbols: a read's length, its words and its counts of symbols are 32 bits wide, its sums are not)
        const uint8_t *s = text + a, *sq = qual + a;
        const uint32_t L0 = (uint32_t)L;
        const uint32_t n_words = (L0 >> 6) + ((L0 & 63u) != 0u);
        uint32_t gc = 0u, acgt = 0u;
        uint64_t qs = 0u;
        uint32_t cc = c0, cn = c1, qc = q0, qn = q1;
        for (uint32_t w = 0; w < n_words; ++w) {
            uint32_t c2 = 0u, q2 = 0u;
            if (w + 2u < n_words) {                                        // (on its way while this word is worked on)
                c2 = read_load(s, L0, ((uint64_t)w + 2u) * 64u + lane);
                if (QUAL) q2 = read_load(sq, L0, ((uint64_t)w + 2u) * 64u + lane);
            }
            const uint32_t base = w * 64u;                                 // (below L0)
            const uint64_t valid = low_bits(L0 - base);
            const uint32_t c = cc & 0xDFu;                                 // (lower case is its base)
            const BaseWords R = base_words(cc);
            const uint64_t RA = R.b[0], RC = R.b[1], RG = R.b[2], RT = R.b[3], any = RA | RC | RG | RT;
            gc += (uint32_t)qc_pop(RC | RG);
            acgt += (uint32_t)qc_pop(any);
            // the lanes of this word at and behind n_pos: the pool's
            const uint64_t pm = valid & ~low_bits(n_pos > base ? n_pos - base : 0u);
            uint32_t mine = 0u;                                            // lane k < 8: this word's count for the pool's counter k
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
            if (base < n_pos) {                                            // the rows of their own: LDS adds, lanes with p < min(L, n_pos)
                const uint32_t p = base + lane;
                if (p < n_pos && p < L0) {
                    // A C G T other = 0 .. 4 from the compares the ballots made (a chain of ?: on c compiles to divergent branches a word)
                    const uint32_t cls = 4u - 4u * (uint32_t)(c == 'A') - 3u * (uint32_t)(c == 'C') - 2u * (uint32_t)(c == 'G') - (uint32_t)(c == 'T');
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
        if (lane == 0u) {                                                  // one add per read and histogram
            atomicAdd(&lds[H + (L0 < n_pos ? L0 : n_pos)], 1u);
            if (acgt) atomicAdd(&lds[H + n_pos + 1u + (uint32_t)(100ull * gc / acgt)], 1u);
            if (QUAL && L0) atomicAdd(&lds[H + n_pos + 1u + 101u + (uint32_t)(qs / L0)], 1u);
        }
    });
    __syncthreads();
    if (threadIdx.x < 8u && pool[threadIdx.x]) atomicAdd(&tables[8u * n_pos + threadIdx.x], pool[threadIdx.x]);
    for (uint32_t i = threadIdx.x; i < H + n_hist; i += RD_WG) {
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
    const uint32_t grid = rd_grid(n_docs);
    if (!grid) return;
    const uint32_t P64 = (n_pos + 63u) & ~63u;
    const size_t lds_bytes = 64u + (8u * (size_t)P64 + n_pos + 1u + 101u + 256u) * 4u;
    if (qual) k_qc_reads<true><<<grid, RD_WG, lds_bytes, st>>>(text, qual, doc_off, n_docs, n_pos, (unsigned long long *)tables);
    else k_qc_reads<false><<<grid, RD_WG, lds_bytes, st>>>(text, nullptr, doc_off, n_docs, n_pos, (unsigned long long *)tables);
}

} // namespace lime
