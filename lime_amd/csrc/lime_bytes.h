// lime_bytes.h -- what the kernels that walk raw file bytes share (lime_fasta_kernel.hip, lime_fastq_kernel.hip, lime_fqtrim_kernel.hip,
// lime_seqcut_kernel.hip): the block geometry, a lane's piece of the input and its per-byte class masks, the workgroup sum over the
// waves' prefix sums, and the write-out of a block's selected bytes through LDS.  Device code (and the launchers' grid size); every
// function is inlined into its caller.  The input is cut into blocks of LIME_FASTA_BLOCK bytes, one workgroup pass each, a lane on 16
// consecutive bytes.  No byte outside [0, n) is loaded: a 16-byte load is issued only where all 16 bytes are inside, the byte in front
// of a lane's piece only where its position is > 0.  Plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_hip.h"
#include "lime_wave.h"

namespace lime {

constexpr int BY_WG = 256;
constexpr uint32_t BY_LANE = 16;                 // bytes one lane handles per block
constexpr uint32_t BY_WAVES = BY_WG / 64;
static_assert(LIME_FASTA_BLOCK == BY_WG * BY_LANE, "a workgroup pass is one block");
constexpr uint32_t BY_BLOCKS = 8192;             // grids are capped and every kernel strides

inline uint32_t by_grid(uint32_t n_blocks) { return n_blocks < BY_BLOCKS ? n_blocks : BY_BLOCKS; }

// the lane's piece [pos, pos + len) of b[0 .. n): bytes past len read as 0
__device__ __forceinline__ uint32_t load_piece(const uint8_t *b, uint64_t n, uint64_t pos, uint32_t w[4])
{
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (pos >= n) return 0u;
    if (pos + BY_LANE <= n) {
        uint4 v;
        __builtin_memcpy(&v, b + pos, 16);                                  // (the input may sit at any alignment)
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return BY_LANE;
    }
    const uint32_t len = (uint32_t)(n - pos);
#pragma unroll
    for (uint32_t j = 0; j < BY_LANE; ++j)
        if (j < len) w[j >> 2] |= (uint32_t)b[pos + j] << ((j & 3u) * 8u);
    return len;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t w[4], uint32_t j) { return (w[j >> 2] >> ((j & 3u) * 8u)) & 255u; }

// bit j: byte j of the piece at pos is line-first, from the piece's '\n' mask and the byte in front of the piece
__device__ __forceinline__ uint32_t line_first(const uint8_t *b, uint64_t pos, uint32_t len, uint32_t nl)
{
    uint32_t first = 0u;                         // byte 0 of the input reads nothing in front of it
    if (len) first = pos == 0 ? 1u : (uint32_t)(b[pos - 1] == '\n');
    return ((nl << 1) | first) & ((1u << len) - 1u);
}

constexpr uint32_t NO_BYTE = 256u;               // a c0 / c1 that no byte equals

struct ByteMasks {
    uint32_t w[4];                               // the bytes
    uint32_t len;
    uint32_t nl, cr, c0, c1;                     // bit j: byte j is '\n', '\r', the caller's c0, c1
    uint32_t lf;                                 // bit j: byte j is line-first (0 where the caller does not ask for it)
    __device__ __forceinline__ uint32_t in() const { return (1u << len) - 1u; }     // bit j: j < len (len <= 16)
};

// the lane's piece at pos with its masks.  want_lf: line-first too, which reads the byte in front of the piece
__device__ __forceinline__ ByteMasks byte_masks(const uint8_t *b, uint64_t n, uint64_t pos, bool want_lf, uint32_t c0 = NO_BYTE, uint32_t c1 = NO_BYTE)
{
    ByteMasks p;
    p.len = load_piece(b, n, pos, p.w);
    p.nl = p.cr = p.c0 = p.c1 = 0u;
#pragma unroll
    for (uint32_t j = 0; j < BY_LANE; ++j) {
        const uint32_t ch = byte_of(p.w, j);
        p.nl |= (uint32_t)(ch == '\n') << j;
        p.cr |= (uint32_t)(ch == '\r') << j;
        p.c0 |= (uint32_t)(ch == c0) << j;
        p.c1 |= (uint32_t)(ch == c1) << j;
    }
    const uint32_t in = p.in();
    p.nl &= in; p.cr &= in; p.c0 &= in; p.c1 &= in;
    p.lf = want_lf ? line_first(b, pos, p.len, p.nl) : 0u;
    return p;
}

// ---- the workgroup sum: lane 63 of every wave posts its wave_incl_scan value to s_sum[wave], a __syncthreads follows, then ----
// v + s_sum[0] + .. + s_sum[n_waves - 1].  With the lane's own wave and the sum in front of the lane within its wave: the sum in front of
// the lane within the block; with BY_WAVES: the block's total.  (The post is one line at each site, and the count is an argument: with a
// helper for the post, or one per count, the compiler orders the callers' code differently.)
__device__ __forceinline__ uint32_t add_waves(const uint32_t (&s_sum)[BY_WAVES], uint32_t n_waves, uint32_t v = 0u)
{
    for (uint32_t k = 0; k < n_waves; ++k) v += s_sum[k];
    return v;
}

// ---- the write-out: a block's selected bytes through s_stage[LIME_FASTA_BLOCK / 16 + 1], placed as in the output modulo 16 ----
// stage[shift .. shift + n) goes to dst[shift ..), dst 16-byte aligned: 16-byte pieces that are whole, bytes at the two ends.  Behind the
// __syncthreads that ends the staging
__device__ __forceinline__ void store_staged(const uint4 *s_stage, uint8_t *dst, uint32_t shift, uint32_t n)
{
    const uint8_t *stage = reinterpret_cast<const uint8_t *>(s_stage);
    for (uint32_t c = threadIdx.x; c < LIME_FASTA_BLOCK / 16 + 1; c += BY_WG) {
        const uint32_t lo = c * 16u < shift ? shift : c * 16u, hi = c * 16u + 16u > shift + n ? shift + n : c * 16u + 16u;
        if (lo >= hi) continue;
        if (hi - lo == 16u) *reinterpret_cast<uint4 *>(dst + c * 16u) = s_stage[c];
        else for (uint32_t k = lo; k < hi; ++k) dst[k] = stage[k];
    }
}

} // namespace lime
