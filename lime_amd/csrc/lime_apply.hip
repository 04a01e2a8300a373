// lime_apply.hip -- the apply kernels of the binned update path (hand-written HIP, gfx950, wave64): every 64 KB region of the table
// built in LDS from its records and written once (k_apply from 32-bit records, k_apply_tiles from k_sort_tiles' rows, with the
// clusterChoose endings of modes 1 and 2), the long clusters' update records (k_apply_bigrecs, k_bigrec_count, k_bigrec_scatter),
// k_region_rows, and their launch wrappers.
#define LIME_DEBUG_TU_APPLY         // lime_debug.h: this file defines g_part_pt in a LIME_APPLY_TIMING build
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include "lime_device.h"
#include "lime_kernels.h"
#include "lime_wave.h"
#include "lime_debug.h"
#include "lime_launch.h"

namespace lime {

// k_apply_tiles: k_apply on the output of k_sort_tiles: the region's records are its run in every tile of its bin.
// Wave w takes the tiles w, w + 8, ... of the bin (a lane reads one tile's two index entries), then their runs one after
// the other, four 16-bit records per lane and step from 8-byte-aligned loads (and the 65th group of a run with them); the
// loads of the next four runs are in flight while four are added.
// MODE (round 5; clusterChoose without the table, ClusterBWT_DA.cpp:385-423): 0 -- the finished region is written to the table; 1 -- nothing is
// written: the region's row segments give row maxima and non-zero counts (whole rows: plain stores; rows that cross a region border: atomic max /
// add on the zeroed arrays) and the count of its last segment; 2 -- the regions are built once more and the rows that passed the host's test
// (row_off[r + 1] > row_off[r]) leave their non-zero cells as (idRef, sim) pairs in ascending idRef at pairs[row_off[r] ..] (regions without a passing
// row are skipped before a record is read).  Both need n_refs >= 256 (at most 257 row segments per 64 KB region, a wave each).
// bytes wb .. wb + 3 of a word that lie in [s, e)
__device__ __forceinline__ uint32_t keep_bytes(uint32_t x, uint32_t wb, uint32_t s, uint32_t e)
{
    uint32_t m = 0xFFFFFFFFu;
    if (wb < s) { const uint32_t d = s - wb; m = d >= 4u ? 0u : m << (8u * d); }
    if (wb + 4u > e) { const uint32_t d = e > wb ? e - wb : 0u; m &= d >= 4u ? 0xFFFFFFFFu : ((1u << (8u * d)) - 1u); }
    return x & m;
}
__device__ __forceinline__ uint32_t nz_bytes(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }   // bit 7 of every non-zero byte

// MODE 1 with at most FIN_SEGS row segments per region (n_refs >= 256): every thread looks at its eight 16-byte pieces of the region -- 97 % of
// them are zero on configs[2] --, finds the row segment of a non-zero piece with one multiplication by 1 / n_refs (corrected by one) and adds the
// piece's maximum / non-zero count to the segment's two LDS words; a piece that holds a row border goes byte by byte.  (The first version gave every
// segment to a wave -- 14 segments of 5000 bytes on 8 waves, each a chain of dependent LDS reads and wave reductions: 1.27 ms on configs[2]
// against 0.89 for the kernel that WRITES the table.)
constexpr uint32_t FIN_SEGS = 258;
// the segments' owner threads: whole rows are stored, rows that cross a region border added atomically (the arrays were zeroed); seg_acc is left zero
__device__ __forceinline__ void fin_region_store(uint32_t *seg_acc, const ApplyFin &f, uint32_t region, uint64_t r0, uint32_t o0, uint32_t nseg, uint32_t len)
{
    for (uint32_t j = threadIdx.x; j < nseg; j += APPLY_WG) {
        const uint32_t mx = seg_acc[j], nz = seg_acc[nseg + j];
        seg_acc[j] = 0u; seg_acc[nseg + j] = 0u;
        const uint64_t row = r0 + j, e64 = (uint64_t)(j + 1u) * f.n_refs - o0;
        const bool whole = (j != 0u || o0 == 0u) && e64 <= len;
        if (whole) { f.row_max[row] = mx; f.row_nnz[row] = nz; }
        else { if (mx) atomicMax(&f.row_max[row], mx); if (nz) atomicAdd(&f.row_nnz[row], nz); }
        if (j == nseg - 1u) f.last_nnz[region] = nz;
    }
}
__device__ __forceinline__ void fin_region_rows(uint4 *reg4, uint32_t *seg_acc, const ApplyFin &f, uint32_t region, uint64_t r0, uint32_t o0, uint32_t nseg, uint32_t len)
{
    // (seg_acc is all zero on entry: cleared at the kernel's start, and by the loop at the end of this function behind every use; the region's LDS copy
    // is left all zero too -- a piece that is looked at and not zero is zeroed right there: the next region needs no clearing pass)
    const uint32_t tid = threadIdx.x;
    const float invf = 1.0f / (float)f.n_refs;
    const uint32_t nq = (len + 15u) >> 4;
    for (uint32_t c = tid; c < nq; c += APPLY_WG) {
        const uint4 v = reg4[c];
        if (!(v.x | v.y | v.z | v.w)) continue;
        reg4[c] = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t x0 = o0 + 16u * c;                          // position of the piece's first byte counted from the start of row r0 (< 2^26)
        uint32_t seg = (uint32_t)((float)x0 * invf);
        if (seg * f.n_refs > x0) --seg; else if ((seg + 1u) * f.n_refs <= x0) ++seg;      // (float: off by one at most)
        const uint32_t border = (seg + 1u) * f.n_refs - o0;        // where the next row starts, in region bytes
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if (border >= 16u * c + 16u) {                             // the whole piece lies in one row
            uint32_t m = 0, z = 0;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t a0 = w[i] & 255u, a1 = (w[i] >> 8) & 255u, a2 = (w[i] >> 16) & 255u, a3 = w[i] >> 24;
                const uint32_t m01 = a0 > a1 ? a0 : a1, m23 = a2 > a3 ? a2 : a3, mm = m01 > m23 ? m01 : m23;
                m = mm > m ? mm : m;
                z += (uint32_t)__popc(nz_bytes(w[i]));
            }
            atomicMax(&seg_acc[seg], m); atomicAdd(&seg_acc[nseg + seg], z);
        } else {                                                   // a row border inside (n_refs >= 256: at most one)
            for (uint32_t b = 0; b < 16u; ++b) {
                const uint32_t val = (w[b >> 2] >> (8u * (b & 3u))) & 255u;
                if (!val) continue;
                const uint32_t sg = seg + (16u * c + b >= border ? 1u : 0u);
                atomicMax(&seg_acc[sg], val); atomicAdd(&seg_acc[nseg + sg], 1u);
            }
        }
    }
    __syncthreads();
    fin_region_store(seg_acc, f, region, r0, o0, nseg, len);
}

template <int MODE>
__device__ __forceinline__ void fin_region(const uint4 *reg4, const ApplyFin &f, uint32_t region, uint64_t r0, uint32_t o0, uint32_t nseg, uint32_t len)
{
    constexpr uint32_t NWV = APPLY_WG / 64;
    const uint32_t lane = lane_id(), wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t reg_base = (uint64_t)region << REGION_SHIFT;
    for (uint32_t j = wave; j < nseg; j += NWV) {                 // a wave per row segment: row r0 + j, bytes [s, e) of the region
        const uint64_t row = r0 + j;
        const uint32_t s = j ? (uint32_t)((uint64_t)j * f.n_refs - o0) : 0u;
        const uint64_t e64 = (uint64_t)(j + 1u) * f.n_refs - o0;
        const uint32_t e = e64 < len ? (uint32_t)e64 : len;
        if (MODE == 1) {
            uint32_t mx = 0, nz = 0;
            for (uint32_t c = (s >> 4) + lane; 16u * c < e; c += 64u) {
                uint4 v = reg4[c];
                if (16u * c < s || 16u * c + 16u > e) {
                    v.x = keep_bytes(v.x, 16u * c, s, e); v.y = keep_bytes(v.y, 16u * c + 4u, s, e);
                    v.z = keep_bytes(v.z, 16u * c + 8u, s, e); v.w = keep_bytes(v.w, 16u * c + 12u, s, e);
                }
                if (v.x | v.y | v.z | v.w) {
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i) {
                        const uint32_t a0 = w[i] & 255u, a1 = (w[i] >> 8) & 255u, a2 = (w[i] >> 16) & 255u, a3 = w[i] >> 24;
                        const uint32_t m01 = a0 > a1 ? a0 : a1, m23 = a2 > a3 ? a2 : a3, m = m01 > m23 ? m01 : m23;
                        mx = m > mx ? m : mx;
                        nz += (uint32_t)__popc(nz_bytes(w[i]));
                    }
                }
            }
            mx = wave_max(mx); nz = wave_sum(nz);
            if (lane == 0) {
                const bool whole = (j != 0u || o0 == 0u) && e64 <= len;
                if (whole) { f.row_max[row] = mx; f.row_nnz[row] = nz; }
                else { if (mx) atomicMax(&f.row_max[row], mx); if (nz) atomicAdd(&f.row_nnz[row], nz); }
                if (j == nseg - 1u) f.last_nnz[region] = nz;
            }
        } else {
            const uint64_t p0 = f.row_off[row], p1 = f.row_off[row + 1u];
            if (p1 == p0) continue;                                // the read did not pass (wave-uniform)
            uint64_t run = p0;
            if (j == 0u && o0 != 0u) {                             // the row began in an earlier region: its cells there come first
                const uint32_t k0 = (uint32_t)((row * f.n_refs) >> REGION_SHIFT);
                for (uint32_t kk = k0; kk < region; ++kk) run += f.last_nnz[kk];
            }
            const uint32_t id0 = (uint32_t)(reg_base - row * f.n_refs);      // idRef of the region's byte 0 in this row (wraps for j > 0: added back below)
            for (uint32_t c0 = s >> 4; 16u * c0 < e; c0 += 64u) {
                const uint32_t c = c0 + lane;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (16u * c < e) {
                    v = reg4[c];
                    if (16u * c < s || 16u * c + 16u > e) {
                        v.x = keep_bytes(v.x, 16u * c, s, e); v.y = keep_bytes(v.y, 16u * c + 4u, s, e);
                        v.z = keep_bytes(v.z, 16u * c + 8u, s, e); v.w = keep_bytes(v.w, 16u * c + 12u, s, e);
                    }
                }
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                const uint32_t cnt = (uint32_t)(__popc(nz_bytes(w[0])) + __popc(nz_bytes(w[1])) + __popc(nz_bytes(w[2])) + __popc(nz_bytes(w[3])));
                if (!__ballot(cnt != 0u)) continue;
                const uint32_t incl = wave_incl_scan(cnt);
                uint64_t at = run + (incl - cnt);
                if (cnt) {
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
                        for (uint32_t b = 0; b < 4; ++b) {
                            const uint32_t val = (w[i] >> (8u * b)) & 255u;
                            if (val) { lime_pair_t pr; pr.id_ref = id0 + 16u * c + 4u * i + b; pr.sim = val; f.pairs[at++] = pr; }
                        }
                }
                run += rl32(incl, 63);
            }
        }
    }
}

template <bool WIDE, int MODE> __global__ __launch_bounds__(APPLY_WG) void k_apply_tiles(uint8_t *sim, size_t sim_bytes, const uint16_t *recs16, const uint32_t *tbase,
                                                          const uint16_t *idx, uint32_t bin_shift, uint32_t n_regions, ApplyFin fin, uint32_t lg_in)
{
    constexpr uint32_t RW = (1u << REGION_SHIFT) / 4u;           // words per region
    constexpr uint32_t NWV = APPLY_WG / 64, UR = 4;
    __shared__ uint4 reg4[RW / 4];
    __shared__ uint32_t seg_acc[MODE == 1 ? 2 * FIN_SEGS : 2];   // MODE 1: maximum and non-zero count of the region's row segments
    // MODE 1: every wave queues the cells its adds found at 0 -- each non-zero cell of the region exactly once, as long as none wraps (a wrap raises
    // ovf_s and the region is rebuilt) -- and the look at the region is a walk over those queues instead of over 64 KB (below)
    constexpr uint32_t QW = 768;                                 // cells a wave can queue per region (more: the region is looked at piece by piece); two workgroups per CU: 64 + 12 + 2 KB each
    __shared__ uint16_t cell_q[MODE == 1 ? NWV * QW : 2];
    __shared__ uint32_t qovf_s[2];                               // by the parity of the workgroup's region count: set during a region's adds, read behind them, cleared a region later
    uint32_t par = 0;
    uint32_t qn = 0;                                             // cells in this wave's queue (wave-uniform)
    uint32_t pf = 0, po01 = 0, po23 = 0;                         // a lane's first adds of the last add4 (a bit each) and their cells, until qflush() queues them
    uint32_t *reg = reinterpret_cast<uint32_t *>(reg4);
    const uint32_t lane = lane_id(), wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: the runs' borders and sources stay scalar
    const uint32_t f2 = 1u << (bin_shift - REGION_SHIFT);
    // one record: + 1 modulo 256 on byte o of the region.  Fast form: ONE returning LDS add of 1 << (8 x byte) on the word -- exact as long
    // as no cell of the word passes 255 (a carry would run into its neighbour); an add that finds its cell at 255 raises the region's
    // flag, and the region is then built again with the exact form, a compare-and-swap per record (real collections never get
    // there: a cell's sum is bounded by the read length; the wrap-around fixtures and the iid generator at few reads do).
    __shared__ uint32_t ovf_s;
    bool exact = false;
    auto add_exact = [&](uint32_t o, uint32_t t = 1u) {
        const uint32_t sh = (o & 3u) * 8u;
        uint32_t *w = &reg[o >> 2];
        uint32_t seen = *w;
        for (;;) {
            const uint32_t b = ((seen >> sh) + t) & 255u;
            const uint32_t old = atomicCAS(w, seen, (seen & ~(255u << sh)) | (b << sh));
            if (old == seen) break;
            seen = old;
        }
    };
    // the four records of a lane's group [p, p + 4), those inside [fa, fe) only.  The four adds leave together and are looked at together: a
    // record outside the run adds 0 to whatever word its bits name (one add at a time behind its own branch, each waiting for its answer,
    // the adds were 77 % of the kernel's cycles at N = 1e10 and 19 .. 34 % elsewhere: tools/r04_apply_phases.sh)
    // (`on`: MODE 1 calls with all the wave's lanes and says which of them hold a group -- its queue count is wave-uniform state that a call
    // under a divergent branch would leave stale in the lanes that sat out)
    auto add4 = [&](uint32_t p, uint2 w, uint32_t fa, uint32_t fe, bool on = true) {
        const uint32_t o[4] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16};
        if (exact) {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) if (on && p + i >= fa && p + i < fe) add_exact(o[i]);
            return;
        }
        // (the valid slots as a 4-bit mask: lo .. hi of the group; p + 4 > fa and p < fe hold for every group that gets here.  The flag is
        // also raised by an add of 0 that meets a cell at 255 -- harmless: the exact pass follows)
        const uint32_t lo = fa > p ? fa - p : 0u, hi = fe - p < 4u ? fe - p : 4u;
        const uint32_t m = on ? ((1u << hi) - 1u) & (~0u << lo) : 0u;
        uint32_t old[4], sh[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            sh[i] = (o[i] << 3) & 24u;
            old[i] = atomicAdd(&reg[o[i] >> 2], ((m >> i) & 1u) << sh[i]);
        }
        bool over = false;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) over |= __builtin_amdgcn_ubfe(old[i], sh[i], 8u) == 255u;
        if (over) ovf_s = 1u;
        if (MODE == 1) {                                          // first adds to their cells: noted here, queued by qflush() -- the callers' lanes differ, and
            pf = 0u;                                              // the queue's count is wave-uniform state that must be kept by ALL lanes
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) pf |= (uint32_t)(((m >> i) & 1u) != 0u && __builtin_amdgcn_ubfe(old[i], sh[i], 8u) == 0u) << i;
            po01 = o[0] | (o[1] << 16); po23 = o[2] | (o[3] << 16);
        }
    };
    // (called by all lanes of the wave, right behind an add4 under its condition)
    auto qflush = [&]() {
        if (MODE != 1) return;
        uint16_t *myq = cell_q + wave * QW;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const bool first = (pf >> i) & 1u;
            const uint64_t mf = __ballot(first);
            if (first) { const uint32_t at = qn + rank_in(mf); if (at < QW) myq[at] = (uint16_t)((i & 2u ? po23 : po01) >> (16u * (i & 1u))); }
            // (the count is ONE number per wave: taken through a scalar register, not a per-lane copy -- the compiler lets lanes that have no further
            // groups leave the callers' `while (__ballot(..))` loops on their own, and a lane that sat a round out would come back with a stale count and
            // write over queued cells: round 6, the run loop of grouped_runs with 16 runs an instruction lost 60 % of a dense region's cells that way)
            qn = (uint32_t)__builtin_amdgcn_readfirstlane((int)(qn + (uint32_t)__popcll(mf)));
        }
        pf = 0u;
    };
    auto add4c = [&](bool on, uint32_t p, uint2 w, uint32_t fa, uint32_t fe) {
        if (on) add4(p, w, fa, fe);
        qflush();
    };
    static_assert(UR == 4, "a step's four runs share one pass over their groups 64 .. 79: sixteen lanes each");
    struct Step { uint2 v[UR], v2[UR], vx; uint32_t fa[UR], fe[UR], q[UR], fax, fex, qx; const uint16_t *src[UR]; };
    if (threadIdx.x == 0) { ovf_s = 0u; qovf_s[0] = 0u; qovf_s[1] = 0u; }
    // A workgroup walks regions blockIdx.x, + gridDim.x, ... (two workgroups per CU).  What a region needs before its records
    // can be read -- its bin's tile range, then its index entries -- is fetched while the region before it is worked on: a
    // workgroup per region paid that chain of dependent loads per region (configs[2]: 76 k regions of 1.6 k records each).
    const uint32_t bsh = bin_shift - REGION_SHIFT;
    auto index_of = [&](uint32_t r, uint32_t r0, uint32_t nr, uint32_t outer, uint32_t &a_, uint32_t &e_) {   // lane l: the index entries of tile outer + wave + NWV * l of the region's bin
        const uint32_t t = outer + wave + NWV * lane;
        a_ = 0u; e_ = 0u;
        if (t < nr) { const uint16_t *ia = idx + (size_t)(r0 + t) * (f2 + 1u) + (r & (f2 - 1u)); a_ = ia[0]; e_ = ia[1]; }      // (tile-major: the lanes' entries lie a tile's f2 + 1 apart; the 64 regions an XCD works on at a time share their lines)
    };
    auto runs_of = [&](uint32_t nr, uint32_t outer) {             // tiles of this round: the wave's are wave, wave + NWV, ... < left
        const uint32_t left = nr - outer;
        return left > wave ? ((left - wave + NWV - 1u) / NWV < 64u ? (left - wave + NWV - 1u) / NWV : 64u) : 0u;
    };
    auto load_step = [&](uint32_t l0, Step &s, uint32_t a_, uint32_t e_, uint32_t nl_, uint32_t row_w) {   // the first 256 records of the runs l0 .. l0 + UR of this wave (row_w: the wave's first tile row)
#pragma unroll
        for (uint32_t u = 0; u < UR; ++u) {
            const uint32_t l = l0 + u;
            s.fa[u] = l < nl_ ? rl32(a_, l) : 0u; s.fe[u] = l < nl_ ? rl32(e_, l) : 0u;
            s.q[u] = (s.fa[u] >> 2) + lane;                       // this lane's group of four records
            s.src[u] = recs16 + (size_t)(row_w + NWV * l) * ROW_STRIDE;
            s.v[u] = make_uint2(0u, 0u);
            if (s.q[u] * 4u < s.fe[u]) s.v[u] = *reinterpret_cast<const uint2 *>(s.src[u] + (size_t)s.q[u] * 4u);
            if (!WIDE) {                                          // the run's 65th group, fetched with the step
                s.v2[u] = make_uint2(0u, 0u);
                if ((s.q[u] + 64u) * 4u < s.fe[u]) s.v2[u] = *reinterpret_cast<const uint2 *>(s.src[u] + (size_t)(s.q[u] + 64u) * 4u);
            }
        }
        // WIDE (many records: chosen at the launch).  The groups 64 .. 79 of the step's four runs, sixteen lanes a run, come with the step and are added in ONE pass: a run is 256 records on
        // average at 32 regions per bin and few start on a group border, so every second run has a 65th group -- fetched when its turn came it
        // was a memory round trip, and added in a pass of its own it cost the instructions of a full pass for one or two lanes.
        if (WIDE) {
            const uint32_t ux = lane >> 4, lx = l0 + ux;
            // (the shuffles by ALL lanes, then the select: under the condition the compiler branches, and a lane reading from a lane the branch
            // has switched off gets 0 -- with 33 .. 63 runs per wave and a last step of fewer than four, the source lanes l0 + ux sit in lane groups
            // whose own run does not exist: the groups 64 .. 79 of the step's runs were dropped, silently -- a bin of 257 .. 511 tiles whose count
            // is not a multiple of 32, e.g. the N = 1e10 series' 307 tiles per bin; found in round 5 by the clustered full-size test)
            const uint32_t sa = (uint32_t)__shfl((int)a_, (int)(lx & 63u)), se = (uint32_t)__shfl((int)e_, (int)(lx & 63u));
            s.fax = lx < nl_ ? sa : 0u; s.fex = lx < nl_ ? se : 0u;
            s.qx = (s.fax >> 2) + 64u + (lane & 15u);
            s.vx = make_uint2(0u, 0u);
            if (s.qx * 4u < s.fex) s.vx = *reinterpret_cast<const uint2 *>(recs16 + (size_t)(row_w + NWV * lx) * ROW_STRIDE + (size_t)s.qx * 4u);
        }
    };
    // Short runs (round 6).  A tile row holds 8192 records of its bin, so a region's run in it has 8192 / (regions per bin) records on average: 256 at 32
    // regions per bin (the N = 1e10 series), 64 at 128 (tables of 10 GB), 16 at 512 -- and with a whole wave per run, a lane a group of four, such runs
    // keep 16 or 4 of the 64 lanes busy: the kernel's time followed the NUMBER of runs, not of records (configs[4]'s shape, clustered: 4.5 ms at 128
    // regions per bin, 7.2 at 256, 13.0 at 512 for the same 1.7e9 records).  Here 2^lg lanes share a run, a lane two groups of four: 64 >> lg runs per
    // instruction, 8 << lg records of each per pass (the mean run x 2); longer runs take further passes.
    const uint32_t lg = lg_in ? lg_in : (f2 >= 512u ? 2u : f2 == 256u ? 3u : f2 == 128u ? 4u : f2 == 64u ? 5u : 6u);      // 6: a wave per run (below)
    struct GStep { uint2 v0, v1; uint32_t fa, fe, q; const uint16_t *src; };
    auto grouped_runs = [&](uint32_t a_, uint32_t e_, uint32_t nl_, uint32_t row_w) {
        const uint32_t LG = 1u << lg, rpi = 64u >> lg, lr_in = lane >> lg, li = lane & (LG - 1u);
        auto gload = [&](uint32_t l0, GStep &s) {
            const uint32_t lr = l0 + lr_in;
            const uint32_t sa = (uint32_t)__shfl((int)a_, (int)(lr & 63u)), se = (uint32_t)__shfl((int)e_, (int)(lr & 63u));      // (by all lanes, the select behind)
            const bool valid = lr < nl_;
            s.fa = valid ? sa : 0u; s.fe = valid ? se : 0u;
            s.q = (s.fa >> 2) + 2u * li;                          // this lane's two groups of four: q, q + 1
            s.src = recs16 + (size_t)(row_w + NWV * (valid ? lr : 0u)) * ROW_STRIDE;
            s.v0 = make_uint2(0u, 0u); s.v1 = make_uint2(0u, 0u);
            if (s.q * 4u < s.fe) s.v0 = *reinterpret_cast<const uint2 *>(s.src + (size_t)s.q * 4u);
            if ((s.q + 1u) * 4u < s.fe) s.v1 = *reinterpret_cast<const uint2 *>(s.src + (size_t)(s.q + 1u) * 4u);
        };
        GStep nxt;
        gload(0u, nxt);
        for (uint32_t l0 = 0; l0 < nl_; l0 += rpi) {
            const GStep cur = nxt;
            if (l0 + rpi < nl_) gload(l0 + rpi, nxt);              // the next runs' loads go out before these are added
            add4c(cur.q * 4u < cur.fe, cur.q * 4u, cur.v0, cur.fa, cur.fe);
            add4c((cur.q + 1u) * 4u < cur.fe, (cur.q + 1u) * 4u, cur.v1, cur.fa, cur.fe);
            for (uint32_t q = cur.q + 2u * LG; __ballot(q * 4u < cur.fe); q += 2u * LG) {      // runs beyond 8 << lg records
                uint2 w0 = make_uint2(0u, 0u), w1 = make_uint2(0u, 0u);
                if (q * 4u < cur.fe) w0 = *reinterpret_cast<const uint2 *>(cur.src + (size_t)q * 4u);
                if ((q + 1u) * 4u < cur.fe) w1 = *reinterpret_cast<const uint2 *>(cur.src + (size_t)(q + 1u) * 4u);
                add4c(q * 4u < cur.fe, q * 4u, w0, cur.fa, cur.fe);
                add4c((q + 1u) * 4u < cur.fe, (q + 1u) * 4u, w1, cur.fa, cur.fe);
            }
        }
    };
    // Workgroup b runs on XCD b % 8 (round-robin dispatch), and the runs of neighbouring regions are neighbours in every tile row -- 32 to 128 bytes each
    // at 128 to 512 regions per bin: with region = b the eight XCDs each fetched the same 128-byte lines into their own L2.  Each XCD takes a block of
    // consecutive regions instead: its 64 resident workgroups work on 64 neighbouring regions at a time.
    uint32_t region = (gridDim.x & 7u) ? blockIdx.x : (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (region >= n_regions) return;
    uint32_t row0 = tbase[region >> bsh], n_rows = tbase[(region >> bsh) + 1u] - row0;
    uint32_t a, e;
    index_of(region, row0, n_rows, 0u, a, e);
    // MODE 1, 2: the region's rows -- first row, offset of the region's first byte in it, row segments, bytes inside the table | (MODE 2: no row of
    // it passed) << 31 -- from k_region_rows' array: a scalar load per region, the next region's in flight while this one is built
    uint4 ri = make_uint4(0u, 0u, 0u, 0u);
    if (MODE != 0) ri = fin.region_rows[region];
    if (MODE == 1) for (uint32_t i = threadIdx.x; i < 2u * FIN_SEGS; i += APPLY_WG) seg_acc[i] = 0u;
    bool clean = false;                                           // the LDS copy is all zero already (MODE 1: the last region's look at it left it so)
    __syncthreads();                                              // (everybody sees the cleared flag)
    AP_DECL
    for (;;) {
        const uint32_t next = region + gridDim.x;
        const bool more = next < n_regions;
        uint32_t nrow0 = 0, nrow1 = 0;                            // the next region's tile range: needed only after this one's records
        if (more) { nrow0 = tbase[next >> bsh]; nrow1 = tbase[(next >> bsh) + 1u]; }
        uint4 nri = make_uint4(0u, 0u, 0u, 0u);
        if (MODE != 0 && more) nri = fin.region_rows[next];
        const bool skip = MODE == 2 && (ri.w >> 31) != 0u;
        if (MODE == 1 && threadIdx.x == 0) qovf_s[par ^ 1u] = 0u;  // (last read a region ago, set again only behind this region's last barrier)
        if (!skip)
        for (exact = false;; exact = true) {                      // once; twice if a cell passed 255 under the fast adds
        qn = 0u;
        if (!(MODE == 1 && clean && !exact)) {
            for (uint32_t i = threadIdx.x; i < RW / 4; i += APPLY_WG) reg4[i] = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
        }
        AP(0)
        for (uint32_t outer = 0; outer < n_rows; outer += NWV * 64u) {
            const uint32_t nl = runs_of(n_rows, outer);
            if (outer || exact) index_of(region, row0, n_rows, outer, a, e);
            // (wave-uniform.  The modes without the table take this path for every group size, a wave per run included: with both paths compiled in they
            // pass 128 registers and a CU holds one workgroup of them instead of two)
            if (MODE != 0 || lg < 6u) { if (nl) grouped_runs(a, e, nl, row0 + outer + wave); continue; }
            Step nxt;
            if (nl) load_step(0u, nxt, a, e, nl, row0 + outer + wave);
            AP(1)
            for (uint32_t l0 = 0; l0 < nl; l0 += UR) {
                AP_WAITVM AP(2)
                Step cur = nxt;
                if (l0 + UR < nl) load_step(l0 + UR, nxt, a, e, nl, row0 + outer + wave);     // the next runs' loads go out before these are added
                AP(3)
                if (WIDE) {
#pragma unroll
                    for (uint32_t u = 0; u < UR; ++u)
                        add4c(cur.q[u] * 4u < cur.fe[u], cur.q[u] * 4u, cur.v[u], cur.fa[u], cur.fe[u]);
                    if (__ballot(cur.qx * 4u < cur.fex)) {
                        add4c(cur.qx * 4u < cur.fex, cur.qx * 4u, cur.vx, cur.fax, cur.fex);
#pragma unroll
                        for (uint32_t u = 0; u < UR; ++u) {        // runs beyond 320 records (groups from 80 on): loaded here, rare
                            const uint32_t fa = cur.fa[u], fe = cur.fe[u];
                            for (uint32_t q = cur.q[u] + 80u; __ballot(q * 4u < fe); q += 64u)
                                { uint2 wq = make_uint2(0u, 0u); if (q * 4u < fe) wq = *reinterpret_cast<const uint2 *>(cur.src[u] + (size_t)q * 4u); add4c(q * 4u < fe, q * 4u, wq, fa, fe); }
                        }
                    }
                } else {
#pragma unroll
                    for (uint32_t u = 0; u < UR; ++u) {
                        uint32_t q = cur.q[u];
                        uint2 w = cur.v[u], w2 = cur.v2[u];
                        const uint32_t fa = cur.fa[u], fe = cur.fe[u];
                        while (__ballot(q * 4u < fe)) {
                            add4c(q * 4u < fe, q * 4u, w, fa, fe);
                            q += 64u;
                            w = w2;
                            if ((q + 64u) * 4u < fe) w2 = *reinterpret_cast<const uint2 *>(cur.src[u] + (size_t)(q + 64u) * 4u);   // (runs beyond 512 records: further groups, loaded here)
                        }
                    }
                }
                AP(4)
            }
        }
        if (MODE == 1 && qn > QW && lane == 0u) qovf_s[par] = 1u;      // (a wave found more first adds than its queue holds: this region is looked at piece by piece)
        __syncthreads();
        AP(5)
        if (exact || !ovf_s) break;
        __syncthreads();                                          // (everybody has seen the flag)
        if (threadIdx.x == 0) ovf_s = 0u;
        }
        if (MODE != 0 && !skip && fin.big_off) {                  // the long clusters' updates of this region (bucketed by region: k_bigrec_*), exact
            const uint64_t lo = fin.big_off[region], hi = fin.big_off[region + 1u];
            for (uint64_t i = lo + threadIdx.x; i < hi; i += APPLY_WG) {
                const uint64_t r = fin.bigrecs[i];
                add_exact((uint32_t)r & ((1u << REGION_SHIFT) - 1u), (uint32_t)(r >> CELL_BITS));
            }
            __syncthreads();
        }
        // the next region's index entries go out now and land while this region is written
        uint32_t na = 0, ne = 0;
        if (more) index_of(next, nrow0, nrow1 - nrow0, 0u, na, ne);
        if (MODE != 0) {
            if (!skip) {
                const uint32_t len = ri.w & 0x7FFFFFFFu;
                clean = false;
                const bool has_big = fin.big_off && fin.big_off[region + 1u] != fin.big_off[region];
                if (MODE == 1 && ri.z <= FIN_SEGS && fin.n_refs >= 16u && !exact && !has_big && qovf_s[par] == 0u) {
                    // the walk over the queued cells: final value of the cell (a byte read), the cell zeroed (a byte store: the LDS copy is left all zero),
                    // its row segment by one multiplication, two LDS adds -- about 30 instructions per 64 cells against 640 per wave for the look at all pieces
                    const uint16_t *myq = cell_q + wave * QW;
                    uint8_t *regb = reinterpret_cast<uint8_t *>(reg4);
                    const float invf = 1.0f / (float)fin.n_refs;
                    for (uint32_t i0 = 0; i0 < qn; i0 += 64u) {
                        const uint32_t i = i0 + lane;
                        if (i < qn) {
                            const uint32_t o = myq[i], val = regb[o];
                            regb[o] = 0;
                            const uint32_t x0 = ri.y + o;
                            uint32_t seg = (uint32_t)((float)x0 * invf);
                            if (seg * fin.n_refs > x0) --seg; else if ((seg + 1u) * fin.n_refs <= x0) ++seg;
                            if (val) { atomicMax(&seg_acc[seg], val); atomicAdd(&seg_acc[ri.z + seg], 1u); }
                        }
                    }
                    __syncthreads();
                    fin_region_store(seg_acc, fin, region, (uint64_t)ri.x, ri.y, ri.z, len);
                    clean = true;
                }
                else if (MODE == 1 && ri.z <= FIN_SEGS && fin.n_refs >= 16u) {
                    fin_region_rows(reg4, seg_acc, fin, region, (uint64_t)ri.x, ri.y, ri.z, len); clean = true;
                }
                else fin_region<MODE>(reg4, fin, region, (uint64_t)ri.x, ri.y, ri.z, len);
            }
        } else {
        const size_t reg_base = (size_t)region << REGION_SHIFT;  // regions start inside the table
        uint4 *dst = reinterpret_cast<uint4 *>(sim + reg_base);
        const size_t left16 = (sim_bytes - reg_base) / 16u;      // sim_bytes is a multiple of 16
        constexpr uint32_t NST = RW / 4 / APPLY_WG;
        static_assert(RW / 4 % APPLY_WG == 0, "whole rounds of 16-byte stores");
        if (left16 >= RW / 4) {
            // the thread's eight 16-byte pieces: read together, then stored together (one after the other every piece waited for its LDS
            // read; named registers, not an array: the array went to scratch memory)
            static_assert(NST == 8, "eight 16-byte stores per thread below");
            uint4 *rp = reg4 + threadIdx.x, *dp = dst + threadIdx.x;
#define LIME_RD(J) const uint4 o##J = rp[J * APPLY_WG];
            LIME_RD(0) LIME_RD(1) LIME_RD(2) LIME_RD(3) LIME_RD(4) LIME_RD(5) LIME_RD(6) LIME_RD(7)
#undef LIME_RD
            // (non-temporal: the table is written once and not read again by the pass -- configs[2] 0.98 -> 0.91 ms, the text workload 83 -> 64 us,
            // configs[4]'s shape 2.06 -> 1.93 ms against plain stores, ABAB in one run)
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define LIME_ST(J) { const u32x4 x = {o##J.x, o##J.y, o##J.z, o##J.w}; __builtin_nontemporal_store(x, reinterpret_cast<u32x4 *>(dp + J * APPLY_WG)); }
            LIME_ST(0) LIME_ST(1) LIME_ST(2) LIME_ST(3) LIME_ST(4) LIME_ST(5) LIME_ST(6) LIME_ST(7)
#undef LIME_ST
        } else {                                                  // the table's last region, cut short (it is its workgroup's last one)
            for (uint32_t i = threadIdx.x; i < left16; i += APPLY_WG) dst[i] = reg4[i];
        }
        }
        AP(6)
        if (!more) break;
        __syncthreads();                                          // (the region's LDS copy has been read: it may be cleared)
        ri = nri; par ^= 1u;
        AP(7)
        region = next; row0 = nrow0; n_rows = nrow1 - nrow0; a = na; e = ne;
    }
    AP_END
}

// k_apply: one workgroup builds one 64 KB region of the table in LDS -- zero, add the region's records (exact
// modulo 256 per byte cell: an LDS compare-and-swap on the containing word), write it out once with 16-byte
// stores.  Two workgroups fit a CU, so one region's write-out overlaps the next one's accumulation.  The table
// needs no clearing beforehand: every byte of it is written here.  Record: offset in its bin | t << bin_shift.
__global__ __launch_bounds__(APPLY_WG) void k_apply(uint8_t *sim, size_t sim_bytes, const uint32_t *recs, const uint64_t *regbase,
                                                    uint32_t bin_shift)
{
    constexpr uint32_t RW = (1u << REGION_SHIFT) / 4u;           // words per region
    __shared__ uint4 reg4[RW / 4];
    uint32_t *reg = reinterpret_cast<uint32_t *>(reg4);
    const uint32_t region = blockIdx.x;
    const size_t reg_base = (size_t)region << REGION_SHIFT;      // grid = regions that start inside the table
    for (uint32_t i = threadIdx.x; i < RW / 4; i += APPLY_WG) reg4[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const uint64_t lo = regbase[region], hi = regbase[region + 1];
    const uint32_t rmask = (1u << REGION_SHIFT) - 1u;
    constexpr uint32_t U = 4;
    for (uint64_t i0 = lo; i0 < hi; i0 += (uint64_t)APPLY_WG * U) {
        uint32_t r[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint64_t i = i0 + (uint64_t)APPLY_WG * u + threadIdx.x;
            r[u] = i < hi ? recs[i] : 0u;                        // t == 0: no record
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t t = r[u] >> bin_shift;
            if (t != 0u) {
                const uint32_t o = r[u] & rmask, sh = (o & 3u) * 8u;
                uint32_t *w = &reg[o >> 2];
                uint32_t seen = *w;
                for (;;) {
                    const uint32_t b = ((seen >> sh) + t) & 255u;
                    const uint32_t old = atomicCAS(w, seen, (seen & ~(255u << sh)) | (b << sh));
                    if (old == seen) break;
                    seen = old;
                }
            }
        }
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(sim + reg_base);
    const size_t left = (sim_bytes - reg_base) / 16u;            // sim_bytes is a multiple of 16
    for (uint32_t i = threadIdx.x; i < RW / 4 && i < left; i += APPLY_WG) dst[i] = reg4[i];     // (non-temporal stores here: no gain, tools/r03_ab2.sh)
}

// the long clusters' updates of ALL ranks (cell | t << CELL_BITS): the ones that fall into this rank's block are added
// to it (exact modulo 256 per byte cell, like k_score_big on a whole table)
__global__ __launch_bounds__(256) void k_apply_bigrecs(const uint64_t *recs, uint64_t n, uint64_t cell_lo, uint64_t cell_hi, uint8_t *block)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        const uint64_t r = recs[i], cell = r & ((1ull << CELL_BITS) - 1ull);
        if (cell >= cell_lo && cell < cell_hi) sim_add(block, cell - cell_lo, (uint32_t)(r >> CELL_BITS));
    }
}

// ---- launch wrappers (host) ------------------------------------------------------------
void launch_apply(uint8_t *sim, size_t sim_bytes, const uint32_t *recs, const uint64_t *regbase, uint32_t bin_shift, hipStream_t st)
{
    const uint32_t grid = (uint32_t)((sim_bytes + ((size_t)1 << REGION_SHIFT) - 1) >> REGION_SHIFT);
    hipLaunchKernelGGL(k_apply, dim3(grid), dim3(APPLY_WG), 0, st, sim, sim_bytes, recs, regbase, bin_shift);
}

// option apply_group (comparison runs): lanes per run of k_apply_tiles as a power of two, 1 .. 6 (6: a wave per run); 0: by the regions per bin
static std::atomic<uint32_t> g_apply_group{0};
void set_apply_group(uint32_t lg) { g_apply_group.store(lg >= 1u && lg <= 6u ? lg : 0u, std::memory_order_relaxed); }
static uint32_t apply_tiles_grid(uint32_t n_regions)
{
    static std::atomic<uint32_t> resident_of[MAX_DEV];           // workgroups that fit the device at once (two per CU: 64 KB of LDS each)
    std::atomic<uint32_t> &slot = resident_of[cur_device()];
    uint32_t resident = slot.load(std::memory_order_relaxed);
    if (!resident) { resident = resident_blocks(k_apply_tiles<false, 0>, APPLY_WG); slot.store(resident, std::memory_order_relaxed); }
    const uint32_t grid = n_regions < resident ? n_regions : resident;
    return grid ? grid : 1u;
}

void launch_apply_tiles_fin(int mode, size_t sim_bytes, uint32_t bin_shift, const uint32_t *tbase, const uint16_t *idx, const uint16_t *out16, bool many_records,
                            const ApplyFin &fin, hipStream_t st)
{
    const uint32_t n_regions = (uint32_t)((sim_bytes + ((size_t)1 << REGION_SHIFT) - 1) >> REGION_SHIFT);
    const dim3 grid(apply_tiles_grid(n_regions)), wg(APPLY_WG);
    if (mode == 1) {
        if (many_records) hipLaunchKernelGGL((k_apply_tiles<true, 1>), grid, wg, 0, st, nullptr, sim_bytes, out16, tbase, idx, bin_shift, n_regions, fin, g_apply_group.load(std::memory_order_relaxed));
        else              hipLaunchKernelGGL((k_apply_tiles<false, 1>), grid, wg, 0, st, nullptr, sim_bytes, out16, tbase, idx, bin_shift, n_regions, fin, g_apply_group.load(std::memory_order_relaxed));
    } else {
        if (many_records) hipLaunchKernelGGL((k_apply_tiles<true, 2>), grid, wg, 0, st, nullptr, sim_bytes, out16, tbase, idx, bin_shift, n_regions, fin, g_apply_group.load(std::memory_order_relaxed));
        else              hipLaunchKernelGGL((k_apply_tiles<false, 2>), grid, wg, 0, st, nullptr, sim_bytes, out16, tbase, idx, bin_shift, n_regions, fin, g_apply_group.load(std::memory_order_relaxed));
    }
}

void launch_apply_by_tiles(uint8_t *sim, size_t sim_bytes, const uint32_t *recs, const uint64_t *binbase, uint32_t n_bins, uint32_t bin_shift,
                           uint32_t *tbase, uint16_t *idx, uint16_t *out16, bool many_records, hipStream_t st, bool big_rows, bool tbase_ready)
{
    launch_sort_tiles(recs, binbase, n_bins, bin_shift, tbase, idx, out16, st, big_rows, tbase_ready);
    const uint32_t n_regions = (uint32_t)((sim_bytes + ((size_t)1 << REGION_SHIFT) - 1) >> REGION_SHIFT);
    const uint32_t grid = apply_tiles_grid(n_regions);
    ApplyFin none; memset(&none, 0, sizeof none);
    // the variant for many records (a step's groups 64 .. 79 in one pass): N = 1e10 (1.2e9 records) 1.09 -> 0.84 ms, configs[4]'s shape (3.2e8)
    // 2.43 -> 2.08; the other one where there are fewer: configs[2] (1.2e8) +3 %, configs[3]'s shape +3 %, text +7 % with the first
    if (many_records) hipLaunchKernelGGL((k_apply_tiles<true, 0>), dim3(grid), dim3(APPLY_WG), 0, st, sim, sim_bytes, out16, tbase, idx, bin_shift, n_regions, none, g_apply_group.load(std::memory_order_relaxed));
    else hipLaunchKernelGGL((k_apply_tiles<false, 0>), dim3(grid), dim3(APPLY_WG), 0, st, sim, sim_bytes, out16, tbase, idx, bin_shift, n_regions, none, g_apply_group.load(std::memory_order_relaxed));
}

// the rows of every 64 KB region of the table (k_apply_tiles, modes 1 and 2): first row, offset of the region's first byte in it, row segments,
// bytes of the region inside the table | (row_off given: none of its rows passed) << 31
__global__ __launch_bounds__(256) void k_region_rows(uint32_t n_regions, uint32_t n_refs, uint64_t table_bytes, const uint64_t *row_off, uint4 *out)
{
    const uint32_t region = blockIdx.x * 256u + threadIdx.x;
    if (region >= n_regions) return;
    const uint64_t rb = (uint64_t)region << REGION_SHIFT;
    const uint32_t len = table_bytes - rb < (1ull << REGION_SHIFT) ? (uint32_t)(table_bytes - rb) : (1u << REGION_SHIFT);
    const uint64_t r0 = rb / n_refs, r1 = (rb + len - 1u) / n_refs;
    const uint32_t skip = row_off && row_off[r1 + 1u] == row_off[r0] ? 1u : 0u;
    out[region] = make_uint4((uint32_t)r0, (uint32_t)(rb - r0 * n_refs), (uint32_t)(r1 - r0) + 1u, len | (skip << 31));
}
void launch_region_rows(uint32_t n_regions, uint32_t n_refs, uint64_t table_bytes, const uint64_t *row_off, void *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_region_rows, dim3((n_regions + 255u) / 256u), dim3(256), 0, st, n_regions, n_refs, table_bytes, row_off, static_cast<uint4 *>(out));
}

// the long clusters' update records bucketed by table region (a few, rarely millions): count, prefix, scatter
__global__ __launch_bounds__(256) void k_bigrec_count(const uint64_t *recs, uint32_t n, uint32_t *cnt)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        atomicAdd(&cnt[(uint32_t)((recs[i] & ((1ull << CELL_BITS) - 1ull)) >> REGION_SHIFT)], 1u);
}
__global__ __launch_bounds__(256) void k_bigrec_scatter(const uint64_t *recs, uint32_t n, const uint64_t *off, uint32_t *cursor, uint64_t *out)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint64_t r = recs[i];
        const uint32_t reg = (uint32_t)((r & ((1ull << CELL_BITS) - 1ull)) >> REGION_SHIFT);
        out[off[reg] + atomicAdd(&cursor[reg], 1u)] = r;
    }
}
void launch_bigrec_buckets(const uint64_t *recs, uint32_t n, uint32_t n_regions, uint32_t *cnt, uint32_t *cursor, uint64_t *off, uint64_t *out, hipStream_t st)
{
    launch_zero2(cnt, (size_t)n_regions * 4u, nullptr, 0, st);
    launch_zero2(cursor, (size_t)n_regions * 4u, nullptr, 0, st);
    const uint32_t grid = n ? ((n + 255u) / 256u < 1024u ? (n + 255u) / 256u : 1024u) : 1u;
    if (n) hipLaunchKernelGGL(k_bigrec_count, dim3(grid), dim3(256), 0, st, recs, n, cnt);
    launch_scan_tiles(cnt, off, n_regions, reinterpret_cast<unsigned long long *>(off + n_regions), st);
    if (n) hipLaunchKernelGGL(k_bigrec_scatter, dim3(grid), dim3(256), 0, st, recs, n, off, cursor, out);
}

void launch_apply_bigrecs(const uint64_t *recs, uint64_t n, uint64_t cell_lo, uint64_t cell_hi, uint8_t *block, hipStream_t st)
{
    if (!n) return;
    const uint64_t want = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_apply_bigrecs, dim3((uint32_t)(want < 4096u ? want : 4096u)), dim3(256), 0, st, recs, n, cell_lo, cell_hi, block);
}

void preload_apply()
{
    (void)apply_tiles_grid(1u << 20);
    preload_kernel(k_apply_tiles<true, 0>); preload_kernel(k_apply);
}

} // namespace lime
