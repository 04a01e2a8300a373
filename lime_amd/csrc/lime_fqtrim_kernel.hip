// lime_fqtrim_kernel.hip -- the quality bytes of four-line FASTQ kept next to the sequences, and the reads cut at both ends by the BWA /
// cutadapt quality rule on the device (lime_docs.cpp sequences the passes; include/lime_hip.h states the rule and what
// lime_quality_trim, the oracle, returns).
//   k_fq_qual      the fourth pass of the FASTQ parse (lime_fastq_kernel.hip; the masks are its passes' own, block_marks of
//                  lime_fastq_marks.h): the quality bytes (ln(i) % 4 == 3, neither '\n' nor '\r') in order to qual[0 ..), through LDS with 16-byte
//                  stores.  The quality bytes in front of block k are off_keep[k] - off_diff[k] modulo 2^32, exactly: both counts are below
//                  2^32.  A malformed input may hold more quality bytes than kept bytes: only qual[0 .. cap) is ever written.
//   k_trim_bounds  per read (lo, hi) by the rule; 16 lanes (one DPP row) on a read, 16 quality bytes a lane, 256 symbols a step, four
//                  reads a wave.  Either end is the same walk over x[t] = q[p(t)] - cutoff, p(t) = t at the 5' end and L - 1 - t at
//                  the 3' end, with the prefix sums P[t]: T = the first t with P[t] > 0 (or L), t* = the first t < T at which P takes
//                  its minimum over [0, T), taken only if that minimum is < 0.  lo = t* + 1 (or 0), hi = L - 1 - t* (or L).  (The 5' end
//                  of the rule is stated with the signs turned: the first sum below 0 and the first maximum above 0.)  A step: each lane
//                  sums its 16 values, a prefix sum over the row gives every lane the sum in front of it, each lane then finds its own
//                  first crossing and first minimum, the lowest crossing lane comes from a ballot and the minimum of the lanes up to it
//                  from a butterfly over the row on (value, t) packed into one word.  Across steps the sum, the minimum, t* and
//                  "stopped" are carried per row, the sums in 64 bits: a read of 10^7 symbols overflows 32.
//   k_trim_copy    text[doc_off[r] + lo .. + len) to its new place, the same 16 lanes on a read, and the new doc_off.
// The block geometry (BY_*), the sum over the waves and the write-out (store_staged) are lime_bytes.h's; row_incl_scan and row_min are lime_wave.h's.
// wave64.  The cross-lane operations (the DPP row prefix sum, the butterfly, the broadcast of a row's total) sit in wave-uniform control
// flow: the loop over the reads depends on blockIdx and the kernel's arguments alone, the loop over a read's steps on a wave maximum
// made scalar, and a row whose read has ended or stopped goes through the steps with nothing to add.  No inline assembly, plain vector
// stores.  No byte outside qual[0 .. n_text) and text[0 .. n_text) is loaded: a 16-byte load only where all 16 bytes are the read's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_wave.h"
#include "lime_bytes.h"
#include "lime_fastq_marks.h"

namespace lime {

namespace {

// off_keep / off_diff: the exclusive sums of k_fq_count's counts.  qual: 16-byte aligned, cap bytes may be written
__global__ void __launch_bounds__(BY_WG) k_fq_qual(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, const uint32_t *off_keep,
                                                   const uint32_t *off_diff, uint8_t *qual, uint64_t cap)
{
    __shared__ uint32_t s_lf[BY_WAVES], s_sum[BY_WAVES];
    __shared__ uint4 s_stage[LIME_FASTA_BLOCK / 16 + 1];                    // the block's quality bytes, placed as in `qual` modulo 16
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_stage);
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        Piece p;
        const uint32_t q = block_marks(b, n, blk, line0, s_lf, p).qual;
        const uint32_t mine = (uint32_t)__builtin_popcount(q), incl = wave_incl_scan(mine);
        if (lane == 63u) s_sum[wave] = incl;
        __syncthreads();
        const uint32_t before = add_waves(s_sum, wave, incl - mine), total = add_waves(s_sum, BY_WAVES);
        const uint32_t base = off_keep[blk] - off_diff[blk], shift = base & 15u;          // the quality bytes in front of the block
        const uint64_t room = (uint64_t)base < cap ? cap - base : 0u;                       // what of qual[base ..) may be written
        const uint32_t n_q = (uint64_t)total < room ? total : (uint32_t)room;
        uint32_t at = shift + before;
#pragma unroll
        for (uint32_t j = 0; j < BY_LANE; ++j)
            if ((q >> j) & 1u) stage[at++] = (uint8_t)(p.w[j >> 2] >> ((j & 3u) * 8u));     // (at most 4096 + 15: inside s_stage)
        __syncthreads();
        store_staged(s_stage, qual + ((uint64_t)base - shift), shift, n_q);                 // stage[shift .. shift + n_q) to qual[base ..)
        __syncthreads();
    }
}

// ---- the trim ----
constexpr uint32_t TR_ROW = 16;                  // lanes on a read: a DPP row
constexpr uint32_t TR_STEP = TR_ROW * 16;        // symbols a row handles per step
constexpr uint32_t TR_READS = BY_WG / TR_ROW;    // reads a workgroup handles per trip
constexpr uint32_t TR_BLOCKS = 1536;             // six workgroups a CU: k_trim_bounds' registers admit seven, and a grid of eight runs its last one alone
constexpr int32_t TR_BIAS = 1 << 20;             // above any sum of a step's 256 values, each in -126 .. 222
constexpr uint32_t TR_NONE = 0xFFFFFFFFu;

// One end of one read, all 16 lanes of its row: q[0 .. L) the read's quality bytes, rev: the 3' end.  -> t* or TR_NONE, the same in every
// lane of the row.  n_steps: wave-uniform, at least ceil(L / TR_STEP) of every row of the wave; cut 0: TR_NONE, nothing is loaded.
__device__ __forceinline__ uint64_t trim_walk(const uint8_t *q, uint64_t L, uint32_t cut, bool rev, uint32_t n_steps)
{
    const uint32_t g = threadIdx.x & (TR_ROW - 1u);
    const int32_t sub = 33 + (int32_t)cut;
    int64_t carry = 0, best = 0;                 // the sum of the steps so far (never above 0 while the walk goes on); the lowest sum so far
    uint64_t ts = ~0ull;
    bool stopped = cut == 0u || L == 0u;
    for (uint32_t s = 0; s < n_steps; ++s) {
        const uint64_t t0 = (uint64_t)s * TR_STEP + g * 16u;               // the lane's 16 values are x[t0 .. t0 + 16)
        const bool live = !stopped && t0 < L;
        // the 16 bytes at p0 = rev ? L - t0 - 16 : t0, those outside [0, L) read as no value (x = 0: behind the read's last value a sum of
        // 0 crosses nothing and is no lower minimum)
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        uint32_t valid = 0u;                     // bit j: byte j of the piece is a value
        if (live) {
            if (t0 + 16u <= L) {
                uint4 v;
                __builtin_memcpy(&v, q + (rev ? L - t0 - 16u : t0), 16);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
                valid = 0xFFFFu;
            } else {
                const uint32_t len = (uint32_t)(L - t0);                    // 1 .. 15 values: at the front of the piece, or (rev) at its back
#pragma unroll
                for (uint32_t j = 0; j < 16u; ++j) {
                    const bool in = rev ? j >= 16u - len : j < len;
                    if (in) {
                        const uint64_t p = rev ? (uint64_t)j - (16u - len) : t0 + j;
                        w[j >> 2] |= (uint32_t)q[p] << ((j & 3u) * 8u);
                        valid |= 1u << j;
                    }
                }
            }
        }
        int32_t x[16];
        int32_t mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {                                // x[k]: the lane's k-th value in walk order
            const uint32_t j = rev ? 15u - k : k;
            const int32_t byte = (int32_t)((w[j >> 2] >> ((j & 3u) * 8u)) & 255u);
            x[k] = (valid >> j) & 1u ? byte - sub : 0;
            mine += x[k];
        }
        const uint32_t incl = row_incl_scan((uint32_t)mine);
        const int32_t front = (int32_t)(incl - (uint32_t)mine);             // the step's sum in front of the lane
        const int32_t total = (int32_t)__shfl((int)incl, (int)(lane_id() | (TR_ROW - 1u)));
        // the lane's own first crossing and first minimum, relative to the step's start: P[t] > 0 <=> front + run > -carry
        const int64_t need = -carry;
        const int32_t thr = need > TR_BIAS ? TR_BIAS : (int32_t)need;       // (no step's sum reaches TR_BIAS)
        int32_t run = front, lmin = 0x7FFFFFFF;
        uint32_t lk = 0u, cross = 16u;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            run += x[k];
            if (cross == 16u && run > thr) cross = k;
            if (cross == 16u && run < lmin) { lmin = run; lk = k; }
        }
        const bool crossed = live && cross < 16u;
        const uint64_t bal = __ballot(crossed);
        const uint32_t row_bits = (uint32_t)(bal >> (lane_id() & ~(TR_ROW - 1u))) & 0xFFFFu;
        const uint32_t first = row_bits ? (uint32_t)__builtin_ctz(row_bits) : TR_ROW;       // the lowest lane of the row that crossed
        // (value, t) of the lane's minimum in one word: the lowest word of the row is the lowest sum at its lowest t
        uint32_t key = TR_NONE;
        if (live && g <= first && lmin != 0x7FFFFFFF) key = ((uint32_t)(lmin + TR_BIAS) << 8) | (g * 16u + lk);
        key = row_min(key);
        if (!stopped && key != TR_NONE) {
            const int64_t v = carry + ((int32_t)(key >> 8) - TR_BIAS);
            if (v < best) { best = v; ts = (uint64_t)s * TR_STEP + (key & 255u); }
        }
        if (first < TR_ROW || (uint64_t)(s + 1u) * TR_STEP >= L) stopped = true;
        else if (!stopped) carry += total;
        if (__builtin_amdgcn_readfirstlane((int)(__ballot(!stopped) != 0ull)) == 0) break;       // every row of the wave has its answer
    }
    return ts;
}

// lo32[r], len32[r] of every read (len32[n_docs] stays as the caller zeroed it); counts[0] += reads that changed, counts[1] += reads with
// symbols that keep none
__global__ void __launch_bounds__(BY_WG) k_trim_bounds(const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t q5, uint32_t q3,
                                                       uint32_t *lo32, uint32_t *len32, unsigned long long *counts)
{
    const uint32_t g = threadIdx.x & (TR_ROW - 1u);
    uint32_t changed = 0u, emptied = 0u;
    for (uint32_t base = blockIdx.x * TR_READS; base < n_docs; base += gridDim.x * TR_READS) {
        const uint32_t r = base + threadIdx.x / TR_ROW;
        uint64_t a = 0u, L = 0u;
        if (r < n_docs) { a = doc_off[r]; L = doc_off[r + 1] - a; }
        const uint64_t steps = (L + TR_STEP - 1u) / TR_STEP;               // (a read holds fewer than 2^32 symbols: 2^24 steps at the most)
        const uint32_t n_steps = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max((uint32_t)steps));
        const uint64_t t5 = trim_walk(qual + a, L, q5, false, n_steps), t3 = trim_walk(qual + a, L, q3, true, n_steps);
        const uint64_t lo = t5 == ~0ull ? 0u : t5 + 1u, hi = t3 == ~0ull ? L : L - 1u - t3;
        const uint64_t len = lo < hi ? hi - lo : 0u;
        if (r < n_docs && g == 0u) {
            lo32[r] = (uint32_t)lo; len32[r] = (uint32_t)len;
            changed += (uint32_t)(len != L);
            emptied += (uint32_t)(L != 0u && len == 0u);
        }
    }
    if (changed) atomicAdd(&counts[0], (unsigned long long)changed);
    if (emptied) atomicAdd(&counts[1], (unsigned long long)emptied);
}

// new_off: the exclusive sum of len32 over n_docs + 1 entries.  out (16-byte aligned, new_off[n_docs] bytes) and out_off[n_docs + 1]
__global__ void __launch_bounds__(BY_WG) k_trim_copy(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const uint32_t *lo32, const uint32_t *len32,
                                                     const uint32_t *new_off, uint8_t *out, uint64_t *out_off)
{
    const uint32_t g = threadIdx.x & (TR_ROW - 1u);
    for (uint32_t base = blockIdx.x * TR_READS; base < n_docs; base += gridDim.x * TR_READS) {
        const uint32_t r = base + threadIdx.x / TR_ROW;
        if (r >= n_docs) continue;
        const uint32_t len = len32[r], to = new_off[r];
        const uint8_t *src = text + doc_off[r] + lo32[r];
        uint8_t *dst = out + to;
        if (g == 0u) {
            out_off[r] = to;
            if (r == n_docs - 1u) out_off[n_docs] = new_off[n_docs];
        }
        for (uint32_t at = g * 16u; at < len; at += TR_STEP) {
            if (at + 16u <= len) {
                uint4 v;
                __builtin_memcpy(&v, src + at, 16);
                __builtin_memcpy(dst + at, &v, 16);
            } else {
                for (uint32_t k = at; k < len; ++k) dst[k] = src[k];
            }
        }
    }
}

} // namespace

void fqt_launch_qual(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *line0, const uint32_t *off_keep, const uint32_t *off_diff, uint8_t *qual,
                     uint64_t cap, hipStream_t st)
{
    if (n_blocks) k_fq_qual<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, line0, off_keep, off_diff, qual, cap);
}

void fqt_launch_bounds(const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t q5, uint32_t q3, uint32_t *lo32, uint32_t *len32,
                       uint64_t *counts, hipStream_t st)
{
    const uint32_t nb = (n_docs + TR_READS - 1u) / TR_READS;
    if (nb) k_trim_bounds<<<nb < TR_BLOCKS ? nb : TR_BLOCKS, BY_WG, 0, st>>>(qual, doc_off, n_docs, q5, q3, lo32, len32, (unsigned long long *)counts);
}

void fqt_launch_copy(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const uint32_t *lo32, const uint32_t *len32, const uint32_t *new_off,
                     uint8_t *out, uint64_t *out_off, hipStream_t st)
{
    const uint32_t nb = (n_docs + TR_READS - 1u) / TR_READS;
    if (nb) k_trim_copy<<<nb < TR_BLOCKS ? nb : TR_BLOCKS, BY_WG, 0, st>>>(text, doc_off, n_docs, lo32, len32, new_off, out, out_off);
}

} // namespace lime
