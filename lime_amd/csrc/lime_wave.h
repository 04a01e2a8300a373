// lime_wave.h -- wave64 and lane primitives of the kernels (gfx950): lane reads and writes, ballot ranks, wave sums and the DPP
// prefix sum, the may_alias types LDS is read and written through, the kernel-argument re-read (cold) and the exact byte add on the
// table.  Device code only; shared by lime_kernels.hip, lime_partition.hip, lime_apply.hip, lime_bytes.h's users, and lime_reads.h with lime_{adapter,filter,overlap,qc}_kernel.hip on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_kernels.h"

namespace lime {

// LDS is written and read through differently typed pointers (bytes as u16/u64, words as uint4):
// these may_alias types keep the compiler from reordering such accesses under type-based aliasing.
typedef volatile uint8_t __attribute__((address_space(3))) lds_vu8;
typedef volatile uint32_t __attribute__((address_space(3))) lds_vu32;
typedef uint16_t __attribute__((may_alias)) u16a;
typedef uint64_t __attribute__((may_alias)) u64a;
typedef uint4 __attribute__((may_alias)) u4a;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
// The kernel's ScanArgs (always its first argument) re-read from the kernarg segment at the point of use: fields that only
// rare paths need (counters, flags, the long-cluster list ...) then cost a scalar load there instead of SGPRs held through
// the whole window loop -- the scan kernels were 2..40 SGPRs over budget and spilled them into VGPR lanes.
__device__ __forceinline__ const ScanArgs &cold(const ScanArgs &)
{
    const ScanArgs __attribute__((address_space(4))) *p = (const ScanArgs __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));                               // opaque: not merged with the by-value copy, not hoisted
    return *(const ScanArgs *)p;
}
__device__ __forceinline__ uint64_t brev64(uint64_t x) { return __builtin_bitreverse64(x); }
__device__ __forceinline__ uint32_t rl32(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
// v with lane L replaced by the wave-uniform value s (this compiler has no v_writelane builtin).  On gfx940/gfx950 a
// vector instruction that reads an SGPR / VCC written by the vector instruction just before it -- here the v_cmp whose
// ballot is s -- needs two wait states.  The compiler's hazard recognizer inserts them for instructions it knows; inline
// assembly is opaque to it, and whenever the scheduler happened to put a bare `v_writelane` right behind its v_cmp it read
// the PREVIOUS ballot: round 2's "wrong cluster counts" of the build with the runtime update-path flag, and round 3's of the
// first lean EBWT=1 binned scan (`v_cmp_gt_u32 vcc, ..` / `v_writelane_b32 v2, vcc_lo, 1` back to back).
// So the wait states are part of the assembly: `s_nop 1` (two wait states) in front, and the four writes of a mask word
// share one statement and one nop.
template <int L> __device__ __forceinline__ uint32_t write_lane(uint32_t v, uint32_t s)
{
    asm("s_nop 1\n\tv_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "n"(L));
    return v;
}
template <int L> __device__ __forceinline__ void write_lane4(uint32_t &v0, uint32_t &v1, uint32_t &v2, uint32_t &v3,
                                                            uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3)
{
    asm("s_nop 1\n\tv_writelane_b32 %0, %4, %8\n\tv_writelane_b32 %1, %5, %8\n\tv_writelane_b32 %2, %6, %8\n\tv_writelane_b32 %3, %7, %8"
        : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3) : "s"(s0), "s"(s1), "s"(s2), "s"(s3), "n"(L));
}
__device__ __forceinline__ uint64_t rl64(uint64_t v, uint32_t l)
{
    return ((uint64_t)rl32((uint32_t)(v >> 32), l) << 32) | rl32((uint32_t)v, l);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int l)
{
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), l) << 32) | (uint32_t)__shfl((int)(uint32_t)v, l);
}
// number of set bits of the wave mask m in lanes below this one (v_mbcnt_lo/hi: two instructions)
__device__ __forceinline__ uint32_t rank_in(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// 32 mask bits starting at bit `pos` of a bit array in LDS (8-byte aligned, at least (pos >> 5) + 2 words long):
// two aligned words and one v_alignbit
typedef uint32_t __attribute__((may_alias)) u32a;
__device__ __forceinline__ uint32_t bits_at(const uint8_t *bits, uint32_t pos)
{
    const u32a *w = reinterpret_cast<const u32a *>(bits) + (pos >> 5);
    return __builtin_amdgcn_alignbit(w[1], w[0], pos & 31u);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// inclusive prefix sum over the 64 lanes with DPP row shifts / row broadcasts (no LDS)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1,3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2,3
    return v;
}

// exact "cell += t (mod 256)" on the byte table through a 32-bit CAS on the containing word.
// First attempt assumes the word is still zero (tables are sparse), then retries on the
// value the CAS returned.
__device__ __forceinline__ void sim_add(uint8_t *sim, uint64_t cell, uint32_t t)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(sim + (cell & ~3ull));
    const uint32_t sh = (uint32_t)(cell & 3ull) * 8u;
    uint32_t expect = 0u;
    for (;;) {
        uint32_t b = ((expect >> sh) + t) & 255u;
        uint32_t want = (expect & ~(255u << sh)) | (b << sh);
        uint32_t old = atomicCAS(w, expect, want);
        if (old == expect) break;
        expect = old;
    }
}

} // namespace lime

namespace lime {

// inclusive prefix sum over the 16 lanes of each DPP row (the first four steps of wave_incl_scan)
__device__ __forceinline__ uint32_t row_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);   // row_shr:8
    return v;
}
// the minimum over the 16 lanes of each row, in every lane of it
__device__ __forceinline__ uint32_t row_min(uint32_t v)
{
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d); v = o < v ? o : v; }
    return v;
}

} // namespace lime
