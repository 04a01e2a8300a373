// lime_fasta_kernel.hip -- FASTA bytes to documents, and the documents' reverse complements, on the device (lime_docs.cpp sequences
// them; include/lime_hip.h states what lime_fasta_read, the oracle, returns).  The host parser's state machine as a rule per byte:
//   byte i is line-first   iff i == 0 or b[i - 1] == '\n'
//   L(i)                   the largest line-first j <= i;   byte i is in a header iff b[L(i)] == '>'
//   byte i is kept         iff b[i] is neither '\n' nor '\r', it is not in a header, and a line-first '>' stands at or before i
//   text = the kept bytes in order;  document k starts at the number of kept bytes before the k-th line-first '>'
// The input is cut into blocks of LIME_FASTA_BLOCK bytes, one workgroup pass each, a lane on 16 consecutive bytes:
//   1  k_fa_lines   per block the last line-first position (+ 1; 0 = none), and the first line-first '>' of the input (atomicMin).
//                   A running maximum over the blocks (rocPRIM, lime_index_sort.hip) gives every block its carry-in L.
//   2  k_fa_count   per block the kept bytes and the header starts.  One exclusive prefix sum each (rocPRIM).
//   3  k_fa_write   the kept bytes through LDS to their places with 16-byte stores, and the doc_off entries.
// Passes 2 and 3 build the same masks (block_masks): 3 reads + at most 1 write per input byte in all.
// The block geometry (BY_*), load_piece, the per-byte masks (byte_masks), the sum over the waves (add_waves) and the write-out (store_staged) are
// lime_bytes.h's, shared with the other kernels over raw file bytes.
// k_fa_revcomp: out[doc_off[d] + k] = comp[in[doc_off[d + 1] - 1 - k]], a lane on 16 consecutive OUTPUT bytes.
// wave64.  The only cross-lane operations are ballots and the DPP prefix sum of lime_wave.h, both in wave-uniform control flow (every
// lane of a workgroup runs every block of its stride loop; a lane past the end holds no bytes).  No inline assembly here, plain
// vector stores.  No byte outside [0, n) and no entry outside doc_off[0 .. n_docs] is loaded: a 16-byte load is issued only where
// all 16 bytes are inside, the byte in front of a lane's piece only where its position is > 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_index.h"
#include "lime_wave.h"
#include "lime_bytes.h"

namespace lime {

namespace {

// the reverse complement's grid cap is the device's resident lanes (256 CUs x 8 waves): more workgroups would only repeat the table's set-up
constexpr uint32_t RC_BLOCKS = 512;
constexpr uint32_t FA_NONE = 0xFFFFFFFFu;        // "no line-first '>'": above every position (n < 2^32)

struct Piece : ByteMasks {                       // with line-first; c0: byte j is '>'
    uint32_t hs;                                 // bit j: byte j is a line-first '>'
};

__device__ __forceinline__ Piece read_piece(const uint8_t *b, uint64_t n, uint64_t pos)
{
    Piece p{byte_masks(b, n, pos, true, '>'), 0u};
    p.hs = p.lf & p.c0;
    return p;
}

// ---- pass 1 ----
__global__ void __launch_bounds__(BY_WG) k_fa_lines(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *last_lf, uint32_t *first_hdr)
{
    __shared__ uint32_t s_last[BY_WAVES], s_first[BY_WAVES];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t pos = (uint64_t)blk * LIME_FASTA_BLOCK + threadIdx.x * BY_LANE;
        const Piece p = read_piece(b, n, pos);
        // pieces are in lane order: the wave's last line-first byte is in the highest lane that has one, its first header in the lowest
        const uint64_t m_lf = __ballot(p.lf != 0u), m_hs = __ballot(p.hs != 0u);
        if (m_lf == 0 ? lane == 0u : lane == 63u - (uint32_t)__builtin_clzll(m_lf))
            s_last[wave] = p.lf ? (uint32_t)pos + (31u - (uint32_t)__builtin_clz(p.lf)) + 1u : 0u;
        if (m_hs == 0 ? lane == 0u : lane == (uint32_t)__builtin_ctzll(m_hs))
            s_first[wave] = p.hs ? (uint32_t)pos + (uint32_t)__builtin_ctz(p.hs) : FA_NONE;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t last = 0u, first = FA_NONE;
            for (uint32_t k = 0; k < BY_WAVES; ++k) {
                if (s_last[k]) last = s_last[k];
                if (first == FA_NONE) first = s_first[k];
            }
            last_lf[blk] = last;
            if (first != FA_NONE) atomicMin(first_hdr, first);
        }
        __syncthreads();
    }
}

// ---- passes 2 and 3: the masks of a block ----
struct Marks { uint32_t keep, hs; };             // bit j: byte j of the lane's piece is kept, is a header start

// cum_lf: the running maximum of pass 1's words (cum_lf[k] - 1 = the last line-first position at or before block k's end)
__device__ __forceinline__ Marks block_masks(const uint8_t *b, uint64_t n, uint32_t blk, const uint32_t *cum_lf, uint32_t first_hdr,
                                             uint32_t *s_has, uint32_t *s_gt, Piece &p)
{
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t pos = (uint64_t)blk * LIME_FASTA_BLOCK + threadIdx.x * BY_LANE;
    p = read_piece(b, n, pos);
    // does the line that reaches into the block start with '>'?  (block 0 starts a line itself; later blocks have byte 0 behind them)
    uint32_t carry = 0u;
    if (blk > 0) { const uint32_t l = cum_lf[blk - 1u]; carry = l ? (uint32_t)(b[l - 1u] == '>') : 0u; }
    // the piece's own last line start, and whether it is a header
    const uint32_t has = p.lf != 0u, top_gt = has ? (p.c0 >> (31u - (uint32_t)__builtin_clz(p.lf | 1u))) & 1u : 0u;
    const uint64_t m_has = __ballot(has != 0u), m_gt = __ballot(top_gt != 0u);
    if (lane == 0u) {
        s_has[wave] = m_has != 0;
        s_gt[wave] = m_has ? (uint32_t)((m_gt >> (63u - (uint32_t)__builtin_clzll(m_has))) & 1u) : 0u;
    }
    __syncthreads();
    uint32_t state = carry;                      // in a header when the piece begins?
    for (uint32_t k = 0; k < wave; ++k) if (s_has[k]) state = s_gt[k];
    const uint64_t below = m_has & ((1ull << lane) - 1ull);
    if (below) state = (uint32_t)((m_gt >> (63u - (uint32_t)__builtin_clzll(below))) & 1u);
    __syncthreads();                             // (s_has / s_gt are written again by the next block)
    uint32_t hdr = 0u;
#pragma unroll
    for (uint32_t j = 0; j < BY_LANE; ++j) {
        if ((p.lf >> j) & 1u) state = (p.c0 >> j) & 1u;
        hdr |= state << j;
    }
    uint32_t after = 0u;                         // bytes at or behind the input's first header start
    if (pos + BY_LANE > first_hdr) after = pos >= first_hdr ? ~0u : ~0u << (uint32_t)(first_hdr - pos);
    Marks m;
    m.keep = p.in() & ~p.nl & ~p.cr & ~hdr & after;
    m.hs = p.hs;
    return m;
}

// kept bytes in the low half, header starts in the high half: a block has at most 4096 and 2048 of them
__device__ __forceinline__ uint32_t packed_counts(const Marks &m) { return (uint32_t)__builtin_popcount(m.keep) | ((uint32_t)__builtin_popcount(m.hs) << 16); }

__global__ void __launch_bounds__(BY_WG) k_fa_count(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *cum_lf, const uint32_t *first_hdr,
                                                    uint32_t *cnt_keep, uint32_t *cnt_hdr)
{
    __shared__ uint32_t s_has[BY_WAVES], s_gt[BY_WAVES], s_sum[BY_WAVES];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t fh = *first_hdr;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        Piece p;
        const Marks m = block_masks(b, n, blk, cum_lf, fh, s_has, s_gt, p);
        const uint32_t incl = wave_incl_scan(packed_counts(m));
        if (lane == 63u) s_sum[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t t = add_waves(s_sum, BY_WAVES);
            cnt_keep[blk] = t & 0xFFFFu;
            cnt_hdr[blk] = t >> 16;
        }
        __syncthreads();
    }
}

// off_keep / off_hdr: the exclusive sums of pass 2's counts, n_blocks + 1 entries (the last one the total)
__global__ void __launch_bounds__(BY_WG) k_fa_write(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *cum_lf, const uint32_t *first_hdr,
                                                    const uint32_t *off_keep, const uint32_t *off_hdr, uint8_t *text, uint64_t *doc_off)
{
    __shared__ uint32_t s_has[BY_WAVES], s_gt[BY_WAVES], s_sum[BY_WAVES];
    __shared__ uint4 s_stage[LIME_FASTA_BLOCK / 16 + 1];                    // the block's kept bytes, placed as in `text` modulo 16
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_stage);
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t fh = *first_hdr;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        Piece p;
        const Marks m = block_masks(b, n, blk, cum_lf, fh, s_has, s_gt, p);
        const uint32_t mine = packed_counts(m), incl = wave_incl_scan(mine);
        if (lane == 63u) s_sum[wave] = incl;
        __syncthreads();
        // kept bytes | header starts of the block in front of this piece, and of the block
        const uint32_t before = add_waves(s_sum, wave, incl - mine), total = add_waves(s_sum, BY_WAVES);
        const uint32_t base = off_keep[blk], shift = base & 15u, n_keep = total & 0xFFFFu;
        uint32_t at = shift + (before & 0xFFFFu);
#pragma unroll
        for (uint32_t j = 0; j < BY_LANE; ++j)
            if ((m.keep >> j) & 1u) stage[at++] = (uint8_t)(p.w[j >> 2] >> ((j & 3u) * 8u));
        uint32_t doc = off_hdr[blk] + (before >> 16);
        for (uint32_t hs = m.hs; hs; hs &= hs - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(hs);
            doc_off[doc++] = (uint64_t)base + (before & 0xFFFFu) + (uint32_t)__builtin_popcount(m.keep & ((1u << j) - 1u));
        }
        __syncthreads();
        store_staged(s_stage, text + (base - shift), shift, n_keep);       // stage[shift .. shift + n_keep) to text[base ..); text is 16-byte aligned
        if (blk == n_blocks - 1u && threadIdx.x == 0) doc_off[off_hdr[n_blocks]] = off_keep[n_blocks];
        __syncthreads();
    }
}

// ---- documents given as arrays: doc_off by lime_build_index's rules (k_idx_check's, which runs together with a pass over the text) ----
__global__ void __launch_bounds__(BY_WG) k_fa_check_off(const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, uint32_t *err)
{
    bool bad = false;
    for (uint64_t k = blockIdx.x * (uint64_t)BY_WG + threadIdx.x; k <= n_docs; k += (uint64_t)gridDim.x * BY_WG) {
        const uint64_t a = doc_off[k];
        if (k == 0 && a != 0) bad = true;
        if (k == n_docs ? a != n_text : a > doc_off[k + 1]) bad = true;
        if (a > n_text) bad = true;
    }
    if (bad) *err = 1u;
}

// ---- reverse complement ----
// lime_fasta_read's table: A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H in both cases, every other byte itself
__device__ __forceinline__ uint8_t complement_of(uint32_t ch)
{
    const uint32_t up = ch & 0xDFu;
    if (up < 'A' || up > 'Z') return (uint8_t)ch;                           // (up in A .. Z only for the letters of either case)
    uint32_t t = up;
    switch (up) {
    case 'A': t = 'T'; break; case 'T': t = 'A'; break; case 'U': t = 'A'; break;
    case 'C': t = 'G'; break; case 'G': t = 'C'; break;
    case 'R': t = 'Y'; break; case 'Y': t = 'R'; break;
    case 'K': t = 'M'; break; case 'M': t = 'K'; break;
    case 'B': t = 'V'; break; case 'V': t = 'B'; break;
    case 'D': t = 'H'; break; case 'H': t = 'D'; break;
    default: break;
    }
    return (uint8_t)(t | (ch & 0x20u));
}

__device__ __forceinline__ uint32_t complement4(const uint8_t *comp, uint32_t w)
{
    return (uint32_t)comp[w & 255u] | ((uint32_t)comp[(w >> 8) & 255u] << 8) | ((uint32_t)comp[(w >> 16) & 255u] << 16) | ((uint32_t)comp[w >> 24] << 24);
}

// doc_off has passed k_fa_check_off's rules (or comes from k_fa_write); n_docs > 0 and n_text > 0
__global__ void __launch_bounds__(BY_WG) k_fa_revcomp(const uint8_t *in, const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, uint8_t *out)
{
    __shared__ uint8_t comp[256];
    comp[threadIdx.x] = complement_of(threadIdx.x);
    __syncthreads();
    const uint64_t n_pieces = (n_text + BY_LANE - 1u) / BY_LANE;
    for (uint64_t c = blockIdx.x * (uint64_t)BY_WG + threadIdx.x; c < n_pieces; c += (uint64_t)gridDim.x * BY_WG) {
        const uint64_t pos = c * BY_LANE;
        const uint32_t len = n_text - pos < BY_LANE ? (uint32_t)(n_text - pos) : BY_LANE;
        // the document of output position pos: the last d with doc_off[d] <= pos (empty documents in front of it are passed over)
        uint64_t lo = 1, hi = n_docs;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (doc_off[mid] > pos) hi = mid; else lo = mid + 1u;
        }
        uint64_t d = lo - 1u, s = doc_off[d], e = doc_off[d + 1u];
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (len == BY_LANE && e >= pos + BY_LANE && e <= n_text && s <= pos) {
            // the whole piece inside one document: its source is 16 consecutive bytes, read backwards
            uint4 v;
            __builtin_memcpy(&v, in + (s + e - pos - BY_LANE), 16);
            w[0] = complement4(comp, __builtin_bswap32(v.w)); w[1] = complement4(comp, __builtin_bswap32(v.z));
            w[2] = complement4(comp, __builtin_bswap32(v.y)); w[3] = complement4(comp, __builtin_bswap32(v.x));
        } else {
#pragma unroll
            for (uint32_t j = 0; j < BY_LANE; ++j) {
                if (j < len) {
                    const uint64_t q = pos + j;
                    while (q >= e && d + 1u < n_docs) { ++d; s = e; e = doc_off[d + 1u]; }
                    const uint64_t src = s + e - 1u - q;
                    const uint32_t ch = src < n_text ? in[src] : 0u;
                    w[j >> 2] |= (uint32_t)comp[ch] << ((j & 3u) * 8u);
                }
            }
        }
        if (len == BY_LANE) *reinterpret_cast<uint4 *>(out + pos) = make_uint4(w[0], w[1], w[2], w[3]);
        else
#pragma unroll
            for (uint32_t j = 0; j < BY_LANE; ++j)
                if (j < len) out[pos + j] = (uint8_t)(w[j >> 2] >> ((j & 3u) * 8u));
    }
}

inline uint32_t blocks_for(uint64_t items, uint32_t cap)
{
    const uint64_t b = (items + BY_WG - 1) / BY_WG;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

} // namespace

void fa_launch_lines(const uint8_t *b, uint64_t n, uint32_t n_blocks, uint32_t *last_lf, uint32_t *first_hdr, hipStream_t st)
{
    if (n_blocks) k_fa_lines<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, last_lf, first_hdr);
}

void fa_launch_count(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *cum_lf, const uint32_t *first_hdr, uint32_t *cnt_keep, uint32_t *cnt_hdr,
                     hipStream_t st)
{
    if (n_blocks) k_fa_count<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, cum_lf, first_hdr, cnt_keep, cnt_hdr);
}

void fa_launch_write(const uint8_t *b, uint64_t n, uint32_t n_blocks, const uint32_t *cum_lf, const uint32_t *first_hdr, const uint32_t *off_keep,
                     const uint32_t *off_hdr, uint8_t *text, uint64_t *doc_off, hipStream_t st)
{
    if (n_blocks) k_fa_write<<<by_grid(n_blocks), BY_WG, 0, st>>>(b, n, n_blocks, cum_lf, first_hdr, off_keep, off_hdr, text, doc_off);
}

void fa_launch_check_off(const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, uint32_t *err, hipStream_t st)
{
    k_fa_check_off<<<blocks_for((uint64_t)n_docs + 1u, 4096u), BY_WG, 0, st>>>(doc_off, n_docs, n_text, err);
}

void fa_launch_revcomp(const uint8_t *in, const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, uint8_t *out, hipStream_t st)
{
    if (n_docs && n_text) k_fa_revcomp<<<blocks_for((n_text + BY_LANE - 1u) / BY_LANE, RC_BLOCKS), BY_WG, 0, st>>>(in, doc_off, n_docs, n_text, out);
}

} // namespace lime
