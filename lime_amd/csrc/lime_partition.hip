// lime_partition.hip -- the partition kernels of the binned update path (hand-written HIP, gfx950, wave64): the scan's 4-byte update
// records into their table bins (k_part, k_part_lines), wide bins on into their regions (k_part2) or into sorted tile rows of 16-bit
// records (k_tile_bases, k_sort_tiles), the regrouping of records received from other ranks (k_regroup), and their launch wrappers.
// The tile size the kernel files agree on (PART_TILE, ROW_STRIDE) is in lime_kernels.h.
#define LIME_DEBUG_TU_PARTITION     // lime_debug.h: this file defines g_part_pt in a LIME_PART_TIMING / LIME_SORT_TIMING build
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <type_traits>
#include "lime_device.h"
#include "lime_kernels.h"
#include "lime_wave.h"
#include "lime_debug.h"
#include "lime_launch.h"

namespace lime {

// (bins as wide as a region: the bin bases are the region bases; wider bins go through k_part2 first)
//
// Both partition kernels move records TILE by TILE through LDS: a tile's records are ranked inside their bin with
// one returning LDS add each, an exclusive scan of the tile's bin counts gives every bin a run of LDS slots, the
// records go to their slots together with their final position, and the tile leaves LDS slot by slot -- so a wave's
// store instruction writes runs of consecutive positions instead of 64 scattered dwords (scattered 4-byte stores
// cost the CU's address path about 3 cycles per lane: 0.8 ms per 1.2e8 records and level, measured).

// exclusive prefix of cnt[0 .. nb) into toff[0 .. nb), nb <= PART_WG * 8; all threads of the workgroup call it
// (barriers inside: cnt is complete on entry, toff on exit)
template <int WG = PART_WG>
__device__ __forceinline__ void part_scan(const uint32_t *cnt, uint32_t *toff, uint32_t nb, uint32_t *wsum)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (nb + WG - 1u) / WG, b0 = tid * per;
    uint32_t mine = 0;
    for (uint32_t k = 0; k < per; ++k) mine += b0 + k < nb ? cnt[b0 + k] : 0u;
    const uint32_t incl = wave_incl_scan(mine);
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    uint32_t run = incl - mine;
    for (uint32_t k = 0; k < wave; ++k) run += wsum[k];
    for (uint32_t k = 0; k < per; ++k) if (b0 + k < nb) { toff[b0 + k] = run; run += cnt[b0 + k]; }
    __syncthreads();
}

// k_part: workgroup p moves the records of producer p (a group of prod_waves scan waves: their pool segments, one after the
// other) into their bins; a record leaves as 4 bytes: cell offset inside the bin | t << bin_shift.  Positions are 32-bit
// (the host keeps a pass below 2^32 records).
// Round 4 (the round-3 kernel issued 60 instructions per 64 records -- 36 vector, 15 scalar, 6 LDS, 2 memory -- and ran at 2.1
// cycles per record and CU whatever the number of bins or of workgroups per CU): (1) a tile is COUNTED per bin (LDS add, nothing
// returned), the counts are scanned, and each record then takes the next slot of its bin's cursor -- the order inside a bin is
// free -- so no rank travels in registers between the passes; (2) records are loaded four at a time (16-byte loads) and the
// tile leaves LDS four slots at a time: consecutive positions go out as ONE 16-byte store (the hardware takes them at any
// 4-byte alignment, tools/store_bench.hip), the others as single words; (3) the bins' global cursors live in the registers of
// the threads that scan them; the counters are cleared by the scan, and the NEXT tile is counted while this one is written
// out: three barriers a tile.
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(4)));   // four words at any 4-byte alignment

// WGS threads and tiles of 16 WGS records: 512 / 8192, or -- few bins: the runs stay long enough -- 256 / 4096 with twice as many
// workgroups per CU: a tile is a chain of short phases between barriers, and what hides their latencies is other workgroups
// P64 (round 5): a pass whose record pool holds 2^32 records or more (N = 1e10 at the update density of real text: 2.4 .. 3.9e9 records) --
// positions in `out` are 64-bit: the bins' cursors are 64-bit registers, a bin's (position - slot) is a 64-bit word in LDS, and the high part
// of a slot's position travels through the stage in the record's free bits above t (t is 1 here: a score of t left the scan as t records),
// bits bin_shift + 1 .. 31: six bits at the widest bins, 2^38 records.  Rounds 1-4 sent such a pass to the compare-and-swap path.
template <int WGS, uint32_t NB_MAX, bool P64>
__global__ __launch_bounds__(WGS) void k_part(ScanArgs a, const uint64_t *binbase, uint32_t *out)
{
    constexpr uint32_t PART_WG = WGS, PART_TILE = WGS * PART_PER, PART_BPT = (NB_MAX + WGS - 1) / WGS;   // (shadow the file's constants)
    __shared__ uint4 stage4[PART_TILE / 2];                              // (position in out, record) per slot
    extern __shared__ __attribute__((aligned(8))) uint32_t part_lds[];   // per bin: tile count, cursor (LDS slot), position - slot (P64: two words)
    __shared__ uint32_t wsum[PART_WG / 64], tile_n_s;
    uint2 *stage = reinterpret_cast<uint2 *>(stage4);
    const uint32_t nb = a.n_bins, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t *cnt = part_lds, *cur = cnt + nb, *delta = cur + nb;
    u64a *delta64 = reinterpret_cast<u64a *>(part_lds + 2u * nb);        // (8-byte aligned: 2 nb words in front; takes the place of delta)
    typedef typename std::conditional<P64, uint64_t, uint32_t>::type pos_t;
    const uint32_t per = (nb + PART_WG - 1u) / PART_WG, b0 = tid * per;
    pos_t G[PART_BPT];                                                   // where this producer's records of bins b0 .. go next
#pragma unroll
    for (uint32_t k = 0; k < PART_BPT; ++k) {
        G[k] = 0u;
        if (k < per && b0 + k < nb) { G[k] = (pos_t)binbase[b0 + k] + a.counts[(size_t)(b0 + k) * gridDim.x + blockIdx.x]; cnt[b0 + k] = 0u; }
    }
    __syncthreads();
    const uint32_t sh = a.bin_shift, omask = (1u << sh) - 1u, tbit = 1u << sh;
    // the producer's segments -- (wave, sub-region): 32-bit records, the cell's high part is the sub-region's number -- as one
    // sequence of tiles
    const uint32_t n_seg = a.prod_waves * a.n_sub, seg0 = blockIdx.x * n_seg;
    // The producer's records -- its (wave, sub-region) pool segments one after the other, each padded to a multiple of four records (16-byte loads,
    // segments start on 64-byte lines) -- are ONE stream cut into tiles of PART_TILE (round 5).  Rounds 3-4 cut every segment into tiles of its own:
    // nothing lost where a segment holds many tiles, but on 10^8-symbol inputs a wave has 800 .. 6000 records and every producer walked 8 partly
    // filled tiles where 1 .. 6 full ones do (configs[1] binned: k_part 52 of the pass's 280 us; the text workload: 8 tiles of 0.72 instead of 5.8).
    // (one word per segment: its padded start | the segment's padding, 0 .. 3 records, in the two low bits -- a second array of counts was the 512 bytes
    // by which k_part_lines<true> at 477 bins no longer fitted a CU twice)
    __shared__ uint32_t segp_s[16u * MAX_SUB + 1u];
    for (uint32_t i = tid; i < n_seg; i += PART_WG) segp_s[i] = a.wave_cnt[seg0 + i];
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < n_seg; ++i) { const uint32_t n = segp_s[i]; segp_s[i] = run | ((0u - n) & 3u); run += (n + 3u) & ~3u; }
        segp_s[n_seg] = run;
    }
    __syncthreads();
    auto seg_p = [&](uint32_t i) { return segp_s[i] & ~3u; };
    auto seg_n = [&](uint32_t i) { const uint32_t w = segp_s[i]; return (segp_s[i + 1u] & ~3u) - (w & ~3u) - (w & 3u); };
    const uint32_t l_pad = segp_s[n_seg];                                // padded records of the producer
    // start in the stream, the segment that holds it; one: the tile's records all lie in that segment (the rule where segments are long: the tile
    // is then described by two wave-uniform words, tn records from the segment's offset v0 - start on, like rounds 3-4's tiles -- the per-group
    // meta words below cost the partition of N = 1e10 6 % when every tile used them)
    struct Tile { uint32_t v0, w0, tn, binoff; bool any, one; };
    auto tile_at = [&](uint32_t v0, uint32_t w0) {
        Tile t; t.v0 = v0; t.w0 = w0; t.any = v0 < l_pad; t.one = false; t.tn = 0u; t.binoff = 0u;
        if (t.any) {
            while (seg_p(t.w0 + 1u) <= v0) ++t.w0;
            const uint32_t end = v0 + PART_TILE < l_pad ? v0 + PART_TILE : l_pad;
            t.one = end <= seg_p(t.w0 + 1u);
            if (t.one) { const uint32_t left = seg_n(t.w0) - (v0 - seg_p(t.w0)); t.tn = left < PART_TILE ? left : PART_TILE; t.binoff = rec_bin_off(t.w0 % a.n_sub, sh); }
        }
        return t;
    };
    auto next_tile = [&](const Tile &c) { return tile_at(c.v0 + PART_TILE, c.w0); };
    // records 4 (j * PART_WG + tid) .. + 3 of the tile (16-byte loads); meta: per group of four how many of them are records (0 .. 4) and the
    // number of their sub-region (= high part of the cell), six bits a group
    auto load_tile = [&](const Tile &t, uint4 (&r)[PART_PER / 4], uint32_t &meta) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        meta = 0u;
        if (t.one) {                                                     // (groups past the tile's end read its last group again: never used, the passes look at tn)
            const u32x4 *src = reinterpret_cast<const u32x4 *>(a.pool + (size_t)(seg0 + t.w0) * a.cap_w + (t.v0 - seg_p(t.w0)));
            const uint32_t lastq = (t.tn - 1u) >> 2;
#pragma unroll
            for (uint32_t j = 0; j < PART_PER / 4; ++j) {
                const uint32_t q = j * PART_WG + tid;
                const u32x4 x = __builtin_nontemporal_load(src + (q < lastq ? q : lastq));
                r[j] = make_uint4(x.x, x.y, x.z, x.w);
            }
            return;
        }
#pragma unroll
        for (uint32_t j = 0; j < PART_PER / 4; ++j) {
            const uint32_t v = t.v0 + 4u * (j * PART_WG + tid);
            r[j] = make_uint4(0u, 0u, 0u, 0u);
            if (v < l_pad) {
                uint32_t w = t.w0;
                while (seg_p(w + 1u) <= v) ++w;
                const uint32_t off = v - seg_p(w), n = seg_n(w), vc = n - off < 4u ? n - off : 4u;
                const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(a.pool + (size_t)(seg0 + w) * a.cap_w + off));
                r[j] = make_uint4(x.x, x.y, x.z, x.w);
                meta |= (vc | ((w % a.n_sub) << 3)) << (6u * j);
            }
        }
    };
    auto count_tile = [&](const Tile &t, const uint4 (&r)[PART_PER / 4], uint32_t meta) {
        if (t.one) {
#pragma unroll
            for (uint32_t j = 0; j < PART_PER / 4; ++j) {
                const uint32_t i = 4u * (j * PART_WG + tid);
                const uint32_t v[4] = {r[j].x, r[j].y, r[j].z, r[j].w};
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) if (i + k < t.tn) atomicAdd(&cnt[rec_bin_at(v[k], sh, t.binoff)], 1u);
            }
            return;
        }
#pragma unroll
        for (uint32_t j = 0; j < PART_PER / 4; ++j) {
            const uint32_t vc = (meta >> (6u * j)) & 7u, bo = rec_bin_off((meta >> (6u * j + 3u)) & 7u, sh);
            const uint32_t v[4] = {r[j].x, r[j].y, r[j].z, r[j].w};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) if (k < vc) atomicAdd(&cnt[rec_bin_at(v[k], sh, bo)], 1u);
        }
    };
    Tile tc = tile_at(0u, 0u);
    if (!tc.any) return;
    uint4 rv[PART_PER / 4], v4[PART_PER / 4];
    uint32_t mv = 0, m4 = 0;                                             // the groups' meta words of rv / v4
    load_tile(tc, rv, mv);
#pragma unroll
    for (uint32_t j = 0; j < PART_PER / 4; ++j) v4[j] = rv[j];
    m4 = mv;
    count_tile(tc, v4, m4);
    Tile tn_ = next_tile(tc);
    if (tn_.any) load_tile(tn_, rv, mv);
    PP_DECL
    for (;;) {
        // ---- scan of the tile's counts: bin cursors (LDS slots), position - slot per bin; the counters go back to zero
        {
            uint32_t c[PART_BPT], mine = 0;
            PP(0)
            __syncthreads();                                             // the counts are complete
            PP(1)
#pragma unroll
            for (uint32_t k = 0; k < PART_BPT; ++k) { c[k] = (k < per && b0 + k < nb) ? cnt[b0 + k] : 0u; mine += c[k]; }
            const uint32_t incl = wave_incl_scan(mine);
            if (lane == 63u) wsum[wave] = incl;
            __syncthreads();
            uint32_t run = incl - mine;
            for (uint32_t k = 0; k < wave; ++k) run += wsum[k];
#pragma unroll
            for (uint32_t k = 0; k < PART_BPT; ++k)
                if (k < per && b0 + k < nb) {
                    cur[b0 + k] = run;
                    if (P64) delta64[b0 + k] = (uint64_t)G[k] - run; else delta[b0 + k] = (uint32_t)G[k] - run;
                    G[k] += c[k]; cnt[b0 + k] = 0u; run += c[k];
                }
            if (tid == PART_WG - 1u) tile_n_s = run;                     // (the last thread's running sum: the tile's records)
            __syncthreads();
            PP(2)
        }
        const uint32_t tile_n = tile_n_s;
        // ---- every record to the next slot of its bin, with its final position
#pragma unroll
        for (uint32_t j = 0; j < PART_PER / 4; ++j) {
            const uint32_t vc = tc.one ? (4u * (j * PART_WG + tid) < tc.tn ? (tc.tn - 4u * (j * PART_WG + tid) < 4u ? tc.tn - 4u * (j * PART_WG + tid) : 4u) : 0u) : (m4 >> (6u * j)) & 7u;
            const uint32_t bo = tc.one ? tc.binoff : rec_bin_off((m4 >> (6u * j + 3u)) & 7u, sh);
            const uint32_t v[4] = {v4[j].x, v4[j].y, v4[j].z, v4[j].w};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (k < vc) {
                    const uint32_t b = rec_bin_at(v[k], sh, bo);
                    const uint32_t slot = atomicAdd(&cur[b], 1u);
                    if (P64) {
                        const uint64_t p = slot + delta64[b];
                        stage[slot] = make_uint2((uint32_t)p, (v[k] & omask) | tbit | (((uint32_t)(p >> 32) << 1) << sh));
                    } else
                    stage[slot] = make_uint2(slot + delta[b], (v[k] & omask) | tbit);      // t = 1
                }
        }
        PP(3)
        __syncthreads();
        PP(4)
        // ---- the next tile is counted now (its records have landed; nobody reads the counters before the next scan) ...
        const Tile tnext = tn_;
        if (tnext.any) {
#pragma unroll
            for (uint32_t j = 0; j < PART_PER / 4; ++j) v4[j] = rv[j];
            m4 = mv;
            count_tile(tnext, v4, m4);
            tn_ = next_tile(tnext);
            if (tn_.any) load_tile(tn_, rv, mv);                         // ... and the one after it is on its way (in front of this tile's stores: behind them -- what helps k_part_lines -- configs[2] 468 -> 497 us: here the stores are many requests, and the loads queue behind them)
        }
        PP(5)
        // ---- ... while this one leaves LDS, four slots a lane: consecutive positions as one 16-byte store
        for (uint32_t q = tid; 4u * q < tile_n; q += PART_WG) {
            const uint4 s0 = stage4[2u * q], s1 = stage4[2u * q + 1u];   // (p0, v0, p1, v1), (p2, v2, p3, v3)
            if (P64) {                                                   // the positions' high parts ride in the records' bits above t
                const uint32_t rm = (tbit << 1) - 1u;
                const uint64_t h0 = (uint64_t)((s0.y >> sh) >> 1) << 32, h1 = (uint64_t)((s0.w >> sh) >> 1) << 32,
                               h2 = (uint64_t)((s1.y >> sh) >> 1) << 32, h3 = (uint64_t)((s1.w >> sh) >> 1) << 32;
                if (4u * q + 3u < tile_n && s1.z == s0.x + 3u && h3 == h0) {
                    u32x4u o = {s0.y & rm, s0.w & rm, s1.y & rm, s1.w & rm};
                    *reinterpret_cast<u32x4u *>(out + (h0 | s0.x)) = o;
                } else {
                    out[h0 | s0.x] = s0.y & rm;
                    if (4u * q + 1u < tile_n) out[h1 | s0.z] = s0.w & rm;
                    if (4u * q + 2u < tile_n) out[h2 | s1.x] = s1.y & rm;
                    if (4u * q + 3u < tile_n) out[h3 | s1.z] = s1.w & rm;
                }
            } else
            if (4u * q + 3u < tile_n && s1.z == s0.x + 3u) {
                u32x4u o = {s0.y, s0.w, s1.y, s1.w};
                *reinterpret_cast<u32x4u *>(out + s0.x) = o;
            } else {
                out[s0.x] = s0.y;
                if (4u * q + 1u < tile_n) out[s0.z] = s0.w;
                if (4u * q + 2u < tile_n) out[s1.x] = s1.y;
                if (4u * q + 3u < tile_n) out[s1.z] = s1.w;
            }
        }
        PP(6)
        if (!tnext.any) break;
        tc = tnext;
    }
    PP_END
}

// k_part_lines: k_part writing WHOLE 64-byte lines.  What bounds the scatter is not its instructions (the leaner kernel above runs
// no faster than round 3's) but the memory side: stores are written through, every (store instruction, 64-byte line) pair is a
// request of its own, and a request that does not cover its line is a read-modify-write at the memory: a tile's run of 7..17
// records per bin costs two of those (tools/store_bench.hip: scattered pieces below 64 bytes write at 0.4 .. 2.9 TB/s, whole
// lines at 7; WRITE_SIZE of round 3's k_part: 1.85 .. 2.06 x its records).  Here every bin keeps the records that do not fill
// a line yet -- at most 15 -- in LDS (64 bytes per bin) until the next tiles complete it: after a producer's first, aligning
// piece of a bin every store to that bin is an aligned 64-byte line (16 lanes), and each line is written once.  Per tile: count
// per bin; scan (per bin: stage cursor, records to emit = up to the last line border, lines = tasks); records to their bins'
// stage slots; one 16-lane group per line writes it from (carry, stage); the bins' owner threads move the tiles' tails into the
// carries.  Needs 64 + 18 bytes of LDS per bin next to the 32 KB stage: up to ~1500 bins (launch_part falls back to k_part).
constexpr uint32_t PL_TASKS = PART_TILE / 16u + 16u;                     // + one task per bin (a first, aligning piece)
// (tasks of a tile: its lines -- at most (PART_TILE + 15 nb) / 16 -- plus one per bin whose first piece is not aligned)
constexpr uint32_t PL_CS = 17;                                          // words per bin's carry row: 16 records on a stride that spreads the bins over the LDS banks (a stride of 16 put every bin's record i on two banks: 77 % of the LDS cycles were bank conflicts)
__host__ __device__ inline size_t part_lines_lds(uint32_t nb, bool p64 = false) { return (size_t)nb * (16u + 4u * PL_CS) + ((size_t)PL_TASKS + 2u * nb) * 4u + (p64 ? 4u * (size_t)nb : 0u); }

template <bool P64>           // P64: 64-bit positions in `out` (see k_part): the bins' cursors are 64-bit registers, a line's lanes read the high word from ghi[bin]
__global__ __launch_bounds__(PART_WG) void k_part_lines(ScanArgs a, const uint64_t *binbase, uint32_t *out)
{
    __shared__ uint4 stage4[PART_TILE / 4];                              // the tile's records, grouped by bin
    extern __shared__ __attribute__((aligned(16))) uint32_t part_lds_al[];
    uint32_t *part_lds = part_lds_al;
    __shared__ uint32_t wsum[PART_WG / 64], n_tasks_s;
    uint32_t *stage = reinterpret_cast<uint32_t *>(stage4);
    const uint32_t nb = a.n_bins, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // dg[b]: (stage start | carried records << 14 | records to emit << 18, position of the bin's next record in out) -- what a line's lanes need
    // of its bin, one 8-byte read; task[j]: bin | line of the bin << 11
    uint32_t *cnt = part_lds, *cur = cnt + nb;
    uint2 *dg = reinterpret_cast<uint2 *>(cur + nb);                     // (8-byte aligned: part_lds is, and cnt + cur are 2 nb words)
    uint32_t *cb = reinterpret_cast<uint32_t *>(dg + nb);                // [nb][PL_CS]: the bins' carried records
    uint32_t *task = cb + (size_t)nb * PL_CS;
    uint32_t *ghi = task + PL_TASKS + 2u * nb;                           // P64: high word of the bin's next position (part_lines_lds(nb, true))
    typedef typename std::conditional<P64, uint64_t, uint32_t>::type pos_t;
    const uint32_t per = (nb + PART_WG - 1u) / PART_WG, b0 = tid * per;
    constexpr uint32_t BPT = 3;                                          // bins a thread owns at most (launch_part: nb <= 3 * PART_WG)
    pos_t G[BPT]; uint32_t C[BPT];                                       // per owned bin: position of its next record in out; records carried
#pragma unroll
    for (uint32_t k = 0; k < BPT; ++k) {
        G[k] = 0u; C[k] = 0u;
        if (k < per && b0 + k < nb) { G[k] = (pos_t)binbase[b0 + k] + a.counts[(size_t)(b0 + k) * gridDim.x + blockIdx.x]; cnt[b0 + k] = 0u; }
    }
    __syncthreads();
    const uint32_t sh = a.bin_shift, omask = (1u << sh) - 1u, tbit = 1u << sh;
    const uint32_t n_seg = a.prod_waves * a.n_sub, seg0 = blockIdx.x * n_seg;
    // (the producer's segments as ONE stream cut into tiles, like k_part)
    // (one word per segment: its padded start | the segment's padding, 0 .. 3 records, in the two low bits -- a second array of counts was the 512 bytes
    // by which k_part_lines<true> at 477 bins no longer fitted a CU twice)
    __shared__ uint32_t segp_s[16u * MAX_SUB + 1u];
    for (uint32_t i = tid; i < n_seg; i += PART_WG) segp_s[i] = a.wave_cnt[seg0 + i];
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < n_seg; ++i) { const uint32_t n = segp_s[i]; segp_s[i] = run | ((0u - n) & 3u); run += (n + 3u) & ~3u; }
        segp_s[n_seg] = run;
    }
    __syncthreads();
    auto seg_p = [&](uint32_t i) { return segp_s[i] & ~3u; };
    auto seg_n = [&](uint32_t i) { const uint32_t w = segp_s[i]; return (segp_s[i + 1u] & ~3u) - (w & ~3u) - (w & 3u); };
    const uint32_t l_pad = segp_s[n_seg];                                // padded records of the producer
    // start in the stream, the segment that holds it; one: the tile's records all lie in that segment (the rule where segments are long: the tile
    // is then described by two wave-uniform words, tn records from the segment's offset v0 - start on, like rounds 3-4's tiles -- the per-group
    // meta words below cost the partition of N = 1e10 6 % when every tile used them)
    struct Tile { uint32_t v0, w0, tn, binoff; bool any, one; };
    auto tile_at = [&](uint32_t v0, uint32_t w0) {
        Tile t; t.v0 = v0; t.w0 = w0; t.any = v0 < l_pad; t.one = false; t.tn = 0u; t.binoff = 0u;
        if (t.any) {
            while (seg_p(t.w0 + 1u) <= v0) ++t.w0;
            const uint32_t end = v0 + PART_TILE < l_pad ? v0 + PART_TILE : l_pad;
            t.one = end <= seg_p(t.w0 + 1u);
            if (t.one) { const uint32_t left = seg_n(t.w0) - (v0 - seg_p(t.w0)); t.tn = left < PART_TILE ? left : PART_TILE; t.binoff = rec_bin_off(t.w0 % a.n_sub, sh); }
        }
        return t;
    };
    auto next_tile = [&](const Tile &c) { return tile_at(c.v0 + PART_TILE, c.w0); };
    // records 4 (j * PART_WG + tid) .. + 3 of the tile (16-byte loads); meta: per group of four how many of them are records (0 .. 4) and the
    // number of their sub-region (= high part of the cell), six bits a group
    auto load_tile = [&](const Tile &t, uint4 (&r)[PART_PER / 4], uint32_t &meta) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        meta = 0u;
        if (t.one) {                                                     // (groups past the tile's end read its last group again: never used, the passes look at tn)
            const u32x4 *src = reinterpret_cast<const u32x4 *>(a.pool + (size_t)(seg0 + t.w0) * a.cap_w + (t.v0 - seg_p(t.w0)));
            const uint32_t lastq = (t.tn - 1u) >> 2;
#pragma unroll
            for (uint32_t j = 0; j < PART_PER / 4; ++j) {
                const uint32_t q = j * PART_WG + tid;
                const u32x4 x = __builtin_nontemporal_load(src + (q < lastq ? q : lastq));
                r[j] = make_uint4(x.x, x.y, x.z, x.w);
            }
            return;
        }
#pragma unroll
        for (uint32_t j = 0; j < PART_PER / 4; ++j) {
            const uint32_t v = t.v0 + 4u * (j * PART_WG + tid);
            r[j] = make_uint4(0u, 0u, 0u, 0u);
            if (v < l_pad) {
                uint32_t w = t.w0;
                while (seg_p(w + 1u) <= v) ++w;
                const uint32_t off = v - seg_p(w), n = seg_n(w), vc = n - off < 4u ? n - off : 4u;
                const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(a.pool + (size_t)(seg0 + w) * a.cap_w + off));
                r[j] = make_uint4(x.x, x.y, x.z, x.w);
                meta |= (vc | ((w % a.n_sub) << 3)) << (6u * j);
            }
        }
    };
    auto count_tile = [&](const Tile &t, const uint4 (&r)[PART_PER / 4], uint32_t meta) {
        if (t.one) {
#pragma unroll
            for (uint32_t j = 0; j < PART_PER / 4; ++j) {
                const uint32_t i = 4u * (j * PART_WG + tid);
                const uint32_t v[4] = {r[j].x, r[j].y, r[j].z, r[j].w};
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) if (i + k < t.tn) atomicAdd(&cnt[rec_bin_at(v[k], sh, t.binoff)], 1u);
            }
            return;
        }
#pragma unroll
        for (uint32_t j = 0; j < PART_PER / 4; ++j) {
            const uint32_t vc = (meta >> (6u * j)) & 7u, bo = rec_bin_off((meta >> (6u * j + 3u)) & 7u, sh);
            const uint32_t v[4] = {r[j].x, r[j].y, r[j].z, r[j].w};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) if (k < vc) atomicAdd(&cnt[rec_bin_at(v[k], sh, bo)], 1u);
        }
    };
    Tile tc = tile_at(0u, 0u);
    if (!tc.any) return;
    uint4 rv[PART_PER / 4], v4[PART_PER / 4];
    uint32_t mv = 0, m4 = 0;                                             // the groups' meta words of rv / v4
    load_tile(tc, rv, mv);
#pragma unroll
    for (uint32_t j = 0; j < PART_PER / 4; ++j) v4[j] = rv[j];
    m4 = mv;
    count_tile(tc, v4, m4);
    Tile tn_ = next_tile(tc);
    if (tn_.any) load_tile(tn_, rv, mv);
    __syncthreads();                                                     // the first tile's counts are complete
    PP_DECL
    for (;;) {
        uint32_t N[BPT], S[BPT], E[BPT], Cold[BPT];
        // ---- scan: per owned bin the tile's records n, with the carried ones T; emit E = up to the last line border reached;
        // L lines = tasks.  One prefix sum over (n | L << 16).
        {
            uint32_t L[BPT], mine = 0;
            PP(0)
            // (no barrier here: the tile was counted in front of the barrier that ended the last write-out, and the carries the owner threads
            // have just moved are read by nobody before three more barriers)
            PP(1)
#pragma unroll
            for (uint32_t k = 0; k < BPT; ++k) {
                N[k] = 0u; E[k] = 0u; L[k] = 0u; Cold[k] = C[k];
                if (k < per && b0 + k < nb) {
                    N[k] = cnt[b0 + k]; cnt[b0 + k] = 0u;
                    const pos_t end = G[k] + C[k] + N[k], border = end & ~(pos_t)15u;
                    if (border > G[k]) { E[k] = (uint32_t)(border - G[k]); L[k] = (uint32_t)((border >> 4) - (G[k] >> 4)); }
                }
                mine += N[k] | (L[k] << 16);
            }
            const uint32_t incl = wave_incl_scan(mine);
            if (lane == 63u) wsum[wave] = incl;
            __syncthreads();
            uint32_t run = incl - mine;
            for (uint32_t k = 0; k < wave; ++k) run += wsum[k];
#pragma unroll
            for (uint32_t k = 0; k < BPT; ++k)
                if (k < per && b0 + k < nb) {
                    const uint32_t b = b0 + k, s0 = run & 0xFFFFu, t0_ = run >> 16;
                    S[k] = s0; cur[b] = s0; dg[b] = make_uint2(s0 | (C[k] << 14) | (E[k] << 18), (uint32_t)G[k]);
                    if (P64) ghi[b] = (uint32_t)((uint64_t)G[k] >> 32);
                    for (uint32_t i = 0; i < L[k]; ++i) task[t0_ + i] = b | (i << 11);
                    G[k] += E[k]; C[k] = C[k] + N[k] - E[k];
                    run += N[k] | (L[k] << 16);
                }
            if (tid == PART_WG - 1u) n_tasks_s = run >> 16;              // (the last thread's running sum is the total)
            __syncthreads();
            PP(2)
        }
        // ---- every record to the next stage slot of its bin
        if (tc.one) {
#pragma unroll
            for (uint32_t j = 0; j < PART_PER / 4; ++j) {
                const uint32_t i = 4u * (j * PART_WG + tid);
                const uint32_t v[4] = {v4[j].x, v4[j].y, v4[j].z, v4[j].w};
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (i + k < tc.tn) stage[atomicAdd(&cur[rec_bin_at(v[k], sh, tc.binoff)], 1u)] = (v[k] & omask) | tbit;      // t = 1
            }
        } else
#pragma unroll
        for (uint32_t j = 0; j < PART_PER / 4; ++j) {
            const uint32_t vc = (m4 >> (6u * j)) & 7u, bo = rec_bin_off((m4 >> (6u * j + 3u)) & 7u, sh);
            const uint32_t v[4] = {v4[j].x, v4[j].y, v4[j].z, v4[j].w};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (k < vc) stage[atomicAdd(&cur[rec_bin_at(v[k], sh, bo)], 1u)] = (v[k] & omask) | tbit;      // t = 1
        }
        PP(3)
        __syncthreads();
        PP(4)
        // ---- the next tile is counted now (only the counters are touched; its records were loaded a tile ago) -- BEFORE this tile's lines are
        // stored: the wait for loaded registers is a wait for every older memory operation of the wave, and right behind the stores it was a wait
        // for their round trip (23 % of the kernel's cycles, tools/r04_part_phases.sh)
        const Tile tnext = tn_;
        if (tnext.any) {
#pragma unroll
            for (uint32_t j = 0; j < PART_PER / 4; ++j) v4[j] = rv[j];
            m4 = mv;
            count_tile(tnext, v4, m4);
        }
        PP(5)
        // ---- a line per 16-lane group: element e of the bin's stream (its carried records, then the tile's) goes to g + e
        {
            // (four lines a turn: each is a chain of dependent LDS reads -- task -> bin -> its descriptors -> the record -- and one at a
            // time the write-out was the longest phase of the kernel)
            constexpr uint32_t GRPS = PART_WG / 16u, UT = 4;
            const uint32_t grp = tid >> 4, l16 = tid & 15u, n_tasks = n_tasks_s;
            for (uint32_t j0 = grp; j0 < n_tasks; j0 += GRPS * UT) {
                uint32_t tt[UT], val[UT], gh[UT];
                pos_t pp[UT];
                uint2 dd[UT];
                bool on[UT];
#pragma unroll
                for (uint32_t u = 0; u < UT; ++u) { const uint32_t j = j0 + u * GRPS; on[u] = j < n_tasks; tt[u] = task[on[u] ? j : 0u]; }
#pragma unroll
                for (uint32_t u = 0; u < UT; ++u) { dd[u] = dg[tt[u] & 0x7FFu]; gh[u] = P64 ? ghi[tt[u] & 0x7FFu] : 0u; }
#pragma unroll
                for (uint32_t u = 0; u < UT; ++u) {
                    const uint32_t bq = tt[u] & 0x7FFu, d = dd[u].x, g = dd[u].y;
                    const uint32_t s0 = d & 0x3FFFu, c = (d >> 14) & 15u, e_n = d >> 18;
                    const uint32_t e = ((tt[u] >> 11) << 4) + l16 - (g & 15u);      // the lane's element of the bin's stream (before the first one: wraps)
                    pp[u] = P64 ? (pos_t)((((uint64_t)gh[u] << 32) | g) + e) : (pos_t)(g + e);      // (e < e_n <= 8207 where it is used: no wrap)
                    on[u] = on[u] && e < e_n;
                    const uint32_t *srcp = e < c ? cb + (bq * PL_CS + e) : stage + (s0 + e - c);
                    val[u] = on[u] ? *srcp : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < UT; ++u) if (on[u]) __builtin_nontemporal_store(val[u], out + pp[u]);      // (whole lines, read once by the next kernel: -1.5 % against plain stores)
            }
        }

        // ---- ... and the tile after it is on its way (behind the stores: by the time its registers are waited for, both are long done)
        if (tnext.any) {
            tn_ = next_tile(tnext);
            if (tn_.any) load_tile(tn_, rv, mv);
        }
        PP(6)
        __syncthreads();                                                 // the lines have been read from the carries and the stage
        // ---- the tails into the carries: a bin that emitted keeps the last C records of the tile, one that did not appends all of them
#pragma unroll
        for (uint32_t k = 0; k < BPT; ++k)
            if (k < per && b0 + k < nb) {
                uint32_t *cbb = cb + (size_t)(b0 + k) * PL_CS;
                if (E[k]) { for (uint32_t i = 0; i < C[k]; ++i) cbb[i] = stage[S[k] + N[k] - C[k] + i]; }
                else      { for (uint32_t i = 0; i < N[k]; ++i) cbb[Cold[k] + i] = stage[S[k] + i]; }
            }
        PP(7)
        if (!tnext.any) break;
        tc = tnext;
    }
    PP_END
    // ---- the end of the producer's records: what the bins still carry (a last, partial line each)
#pragma unroll
    for (uint32_t k = 0; k < BPT; ++k)
        if (k < per && b0 + k < nb) for (uint32_t i = 0; i < C[k]; ++i) out[G[k] + i] = cb[(size_t)(b0 + k) * PL_CS + i];
}

// k_part2: second level, one workgroup per bin (bins wider than a region only): the bin's records are counted per
// 64 KB region of the table, the regions' bases go to regbase[bin * F2 + sub] (F2 = regions per bin), and a second
// sweep (served by the L2: a bin's records are a few hundred KB) moves each record to its region's range of `out`,
// tile by tile through LDS like k_part.
__global__ __launch_bounds__(PART_WG) void k_part2(const uint32_t *recs, const uint64_t *binbase, uint32_t bin_shift,
                                                   uint64_t *regbase, uint32_t *out)
{
    constexpr uint32_t F2MAX = 1u << (BIN_SHIFT_MAX - REGION_SHIFT);
    __shared__ uint2 stage[PART_TILE];
    __shared__ uint32_t cnt[F2MAX], toff[F2MAX], gcur[F2MAX];
    __shared__ uint32_t wsum[PART_WG / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t f2 = 1u << (bin_shift - REGION_SHIFT), omask = (1u << bin_shift) - 1u;
    const uint32_t bin = blockIdx.x;
    const uint64_t lo = binbase[bin], hi = binbase[bin + 1];
    for (uint32_t i = tid; i < f2; i += PART_WG) cnt[i] = 0u;
    __syncthreads();
    // ---- sweep 1: records per region.  Aligned groups of four records (16-byte loads); records outside [lo, hi)
    // read as 0 = no record (t == 0)
    {
        const uint64_t q0 = lo >> 2, q1 = (hi + 3u) >> 2;
        const uint4 *rq = reinterpret_cast<const uint4 *>(recs);
        constexpr uint32_t U = 4;
        for (uint64_t qb = q0; qb < q1; qb += (uint64_t)PART_WG * U) {
            uint4 r[U];
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint64_t q = qb + (uint64_t)PART_WG * u + tid;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (q < q1) {
                    v = rq[q];
                    const uint64_t i = q << 2;
                    if (i < lo || i + 3u >= hi) {
                        v.x = (i >= lo && i < hi) ? v.x : 0u; v.y = (i + 1u >= lo && i + 1u < hi) ? v.y : 0u;
                        v.z = (i + 2u >= lo && i + 2u < hi) ? v.z : 0u; v.w = (i + 3u >= lo && i + 3u < hi) ? v.w : 0u;
                    }
                }
                r[u] = v;
            }
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t wv[4] = {r[u].x, r[u].y, r[u].z, r[u].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) if (wv[k] >> bin_shift) atomicAdd(&cnt[(wv[k] & omask) >> REGION_SHIFT], 1u);
            }
        }
    }
    __syncthreads();
    part_scan(cnt, gcur, f2, wsum);                                  // gcur[sub] = where region sub starts inside the bin
    // words of the bin that are no record (t == 0: a caller of lime_apply_records_dev may pad with them) move nowhere: the regions' ranges fill the
    // bin's first n_valid places, and the rest of it -- which the bin's last region reaches up to, its range ends where the next bin starts -- is
    // written as "no record" here (the array is scratch: what it held is anything)
    const uint32_t n_valid = gcur[f2 - 1u] + cnt[f2 - 1u];
    __syncthreads();
    for (uint32_t i = tid; i < f2; i += PART_WG) { regbase[(size_t)bin * f2 + i] = lo + gcur[i]; cnt[i] = 0u; }
    for (uint64_t i = lo + n_valid + tid; i < hi; i += PART_WG) out[i] = 0u;
    __syncthreads();
    // ---- sweep 2: tile by tile into the regions' ranges (the next tile's records are loaded meanwhile)
    auto load_tile = [&](uint64_t t0, uint32_t (&v)[PART_PER]) {
        const uint32_t tn = hi - t0 < PART_TILE ? (uint32_t)(hi - t0) : PART_TILE;
#pragma unroll
        for (uint32_t j = 0; j < PART_PER; ++j) {
            const uint32_t i = j * PART_WG + tid;
            v[j] = i < tn ? recs[t0 + i] : 0u;
        }
    };
    uint32_t nxt[PART_PER];
    if (lo < hi) load_tile(lo, nxt);
    for (uint64_t t0 = lo; t0 < hi; t0 += PART_TILE) {
        uint32_t val[PART_PER], dr[PART_PER];
#pragma unroll
        for (uint32_t j = 0; j < PART_PER; ++j) {
            val[j] = nxt[j]; dr[j] = ~0u;
            if (val[j] >> bin_shift) {
                const uint32_t d = (val[j] & omask) >> REGION_SHIFT;
                dr[j] = d | (atomicAdd(&cnt[d], 1u) << 12);
            }
        }
        if (t0 + PART_TILE < hi) load_tile(t0 + PART_TILE, nxt);
        __syncthreads();
        part_scan(cnt, toff, f2, wsum);
#pragma unroll
        for (uint32_t j = 0; j < PART_PER; ++j)
            if (dr[j] != ~0u) {
                const uint32_t d = dr[j] & 0xFFFu, r = dr[j] >> 12;
                stage[toff[d] + r] = make_uint2(gcur[d] + r, val[j]);
            }
        __syncthreads();
        const uint32_t nv = toff[f2 - 1u] + cnt[f2 - 1u];               // the tile's records: tn less its no-record words, which were not staged
        for (uint32_t i = tid; i < nv; i += PART_WG) { const uint2 sv = stage[i]; out[lo + sv.x] = sv.y; }
        __syncthreads();
        for (uint32_t i = tid; i < f2; i += PART_WG) { gcur[i] += cnt[i]; cnt[i] = 0u; }
        __syncthreads();
    }
}

// ---- second level without a second sweep -------------------------------------------------------------------------
// k_part2 reads a bin's records twice (count per region, then move) because every region's range of the output must be
// known before the first record moves.  k_sort_tiles does not move records between tiles at all: a bin's records are
// taken TILE by TILE (8192), each tile is sorted by region in LDS and leaves as 16-bit offsets inside the region (the
// region is what the position says), 16 KB per tile at out16[row * PART_TILE ..], row = the tile's number over all bins
// (tbase[bin] + tile of the bin); where the regions' runs start inside the tile goes to the bin's index,
// idx[(tbase[bin] + t) * (f2 + 1) + sub] (t: the tile of the bin; entry f2: the tile's record count).  k_apply_tiles
// then builds a region from its run of every tile of the bin.  One read of 4 bytes and one write of 2 per record here,
// one read of 2 there (k_part2 + k_apply: 8 + 4 and 4).
__global__ __launch_bounds__(PART_WG) void k_tile_bases(const uint64_t *binbase, uint32_t n_bins, uint32_t *tbase)
{
    __shared__ uint32_t cnt[BIN_MAX], toff[BIN_MAX];
    __shared__ uint32_t wsum[PART_WG / 64];
    for (uint32_t b = threadIdx.x; b < n_bins; b += PART_WG) cnt[b] = (uint32_t)((binbase[b + 1] - binbase[b] + PART_TILE - 1u) / PART_TILE);
    __syncthreads();
    part_scan(cnt, toff, n_bins, wsum);
    for (uint32_t b = threadIdx.x; b < n_bins; b += PART_WG) { tbase[b] = toff[b]; if (b == n_bins - 1u) tbase[n_bins] = toff[b] + cnt[b]; }
}

__global__ __launch_bounds__(PART_WG) void k_sort_tiles(const uint32_t *recs, const uint64_t *binbase, uint32_t bin_shift,
                                                        const uint32_t *tbase, uint16_t *idx, uint16_t *out16, uint32_t nt_rows)
{
    constexpr uint32_t F2MAX = 1u << (BIN_SHIFT_MAX - REGION_SHIFT);
    __shared__ uint4 stage4[PART_TILE / 8];                              // the tile's 16-bit offsets, sorted by region
    __shared__ uint32_t cnt[F2MAX], toff[F2MAX];
    __shared__ uint32_t wsum[PART_WG / 64];
    uint16_t *stage = reinterpret_cast<uint16_t *>(stage4);
    const uint32_t tid = threadIdx.x;
    const uint32_t f2 = 1u << (bin_shift - REGION_SHIFT), omask = (1u << bin_shift) - 1u;
    // every region's counter comes in R copies, a lane uses copy lane % R: 64 lanes on 32 counters is what an LDS add is slowest at (10 cycles
    // an instruction against 6.5 on 128 and more, tools/lds_bench.hip), and the ranks were a third of the kernel's cycles (tools/r04_sort_phases.sh).
    // The copies of a region lie next to each other, so the scan hands each its own piece of the region's run.
    const uint32_t rsh = f2 <= 32u ? 4u : f2 <= 64u ? 3u : f2 <= 128u ? 2u : f2 <= 256u ? 1u : 0u, nc = f2 << rsh;      // nc <= F2MAX counters
    const uint32_t mycopy = (threadIdx.x & 63u) & ((1u << rsh) - 1u);
    // workgroup (bin, k) of gridDim.y takes the bin's tiles k, k + gridDim.y, ...: tiles are independent of each other, and a
    // workgroup per BIN left the CUs unevenly loaded (477 or 1193 workgroups of 8 waves over 256 CUs, 292 on the text workload)
    const uint32_t bin = blockIdx.x, kq = blockIdx.y, nq = gridDim.y;
    const uint64_t lo = binbase[bin], hi = binbase[bin + 1];
    const uint32_t row0 = tbase[bin];
    uint16_t *bidx = idx + (size_t)row0 * (f2 + 1u);
    for (uint32_t i = tid; i < nc; i += PART_WG) cnt[i] = 0u;
    __syncthreads();
    const uint64_t step = (uint64_t)PART_TILE * nq, first = lo + (uint64_t)PART_TILE * kq;
    auto load_tile = [&](uint64_t t0, uint32_t (&v)[PART_PER]) {
        const uint32_t tn = hi - t0 < PART_TILE ? (uint32_t)(hi - t0) : PART_TILE;
#pragma unroll
        for (uint32_t j = 0; j < PART_PER; ++j) {
            const uint32_t i = j * PART_WG + tid;
            v[j] = i < tn ? __builtin_nontemporal_load(recs + t0 + i) : 0u;
        }
    };
    uint32_t nxt[PART_PER];
    if (first < hi) load_tile(first, nxt);
    uint32_t row = kq;
    __shared__ uint32_t nv_s;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    ST_DECL
    for (uint64_t t0 = first; t0 < hi; t0 += step, row += nq) {
        ST_WAITVM ST(0)
        uint32_t val[PART_PER], dr[PART_PER];
#pragma unroll
        for (uint32_t j = 0; j < PART_PER; ++j) {
            val[j] = nxt[j]; dr[j] = ~0u;
            if (val[j] >> bin_shift) {                                   // (0: no record)
                const uint32_t d = (((val[j] & omask) >> REGION_SHIFT) << rsh) | mycopy;
                dr[j] = d | (atomicAdd(&cnt[d], 1u) << 12);
            }
        }
        ST(1)
        if (t0 + step < hi) load_tile(t0 + step, nxt);
        ST(2)
        __syncthreads();
        ST(3)
        // the regions' starts inside the tile: f2 <= 512 counters, one per thread; the counters go back to zero right here (round 3 cleared them in
        // a pass of their own behind two more barriers: four barriers a tile now instead of six)
        {
            static_assert(F2MAX <= PART_WG, "a region's counter per thread");
            const uint32_t c = tid < nc ? cnt[tid] : 0u;
            const uint32_t incl = wave_incl_scan(c);
            if (lane == 63u) wsum[wave] = incl;
            __syncthreads();
            uint32_t run = incl - c;
            for (uint32_t k = 0; k < wave; ++k) run += wsum[k];
            // (the tile's f2 + 1 entries lie together -- idx[(row0 + row) * (f2 + 1) + region] --: one or a few whole lines per tile.  Until round 6 the index
            // was region-major, every tile writing f2 + 1 two-byte entries a row stride apart: 0.5 ms of k_sort_tiles' 2.85 at 512 regions per bin)
            if (tid < nc) { toff[tid] = run; cnt[tid] = 0u; if (!(tid & ((1u << rsh) - 1u))) bidx[(size_t)row * (f2 + 1u) + (tid >> rsh)] = (uint16_t)run; }
            if (tid == nc - 1u) { nv_s = run + c; bidx[(size_t)row * (f2 + 1u) + f2] = (uint16_t)(run + c); }
            __syncthreads();
        }
        ST(4)
#pragma unroll
        for (uint32_t j = 0; j < PART_PER; ++j)
            if (dr[j] != ~0u) stage[toff[dr[j] & 0xFFFu] + (dr[j] >> 12)] = (uint16_t)(val[j] & ((1u << REGION_SHIFT) - 1u));
        ST(5)
        __syncthreads();
        ST(6)
        const uint32_t nv = nv_s;                                        // records of the tile
        uint4 *dst = reinterpret_cast<uint4 *>(out16 + (size_t)(row0 + row) * ROW_STRIDE);
        // (whole 16-byte groups: the row is the tile's alone.  Non-temporal where the rows of the pass do not fit the Infinity Cache anyway -- N = 1e10
        // 1.56 -> 1.50 ms and 3 % in k_apply_tiles, configs[4]'s shape 433 -> 391 us --; where they do, plain stores leave them there for
        // k_apply_tiles: the text workload's 48 MB of rows 65 against 101 us in that kernel)
        if (nt_rows) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            for (uint32_t i = tid; i < (nv + 7u) / 8u; i += PART_WG) { const uint4 v = stage4[i]; const u32x4 x = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(x, reinterpret_cast<u32x4 *>(dst + i)); }
        } else
            for (uint32_t i = tid; i < (nv + 7u) / 8u; i += PART_WG) dst[i] = stage4[i];
        // (no barrier here: the next tile's ranks touch the counters only -- cleared above -- and its staging comes behind two barriers)
        ST(7)
    }
    ST_END
}

// =========================================================================================
// Owner-partitioned exchange of table updates (several GPUs, large tables): every rank leaves its updates as records
// grouped by table bin (k_part); the owner of a range of bins receives, from every rank, the slice of records of its
// bins and builds ITS block of the table alone.  k_regroup: the received slices (source-major, each grouped by bin) into
// one array grouped by bin -- a workgroup per bin copies the sources' runs one after the other.
// srcoff[s * (nb + 1) + b]: where source s's records of local bin b start in rx; dstbase[b]: where bin b starts in dst.
// =========================================================================================
__global__ __launch_bounds__(256) void k_regroup(const uint32_t *rx, const uint64_t *srcoff, uint32_t n_src, uint32_t nb,
                                                 const uint64_t *dstbase, uint32_t *dst)
{
    const uint32_t b = blockIdx.x;
    uint64_t at = dstbase[b];
    for (uint32_t s = 0; s < n_src; ++s) {
        const uint64_t lo = srcoff[(size_t)s * (nb + 1u) + b], hi = srcoff[(size_t)s * (nb + 1u) + b + 1u];
        for (uint64_t i = lo + threadIdx.x; i < hi; i += 256u) dst[at + (i - lo)] = rx[i];
        at += hi - lo;
    }
}

// ---- launch wrappers (host) ------------------------------------------------------------
void launch_part(const ScanArgs &a, uint32_t n_prod, const uint64_t *binbase, uint32_t *out, hipStream_t st, bool p64, bool lines_ok)
{
    static std::atomic<bool> attr_set[MAX_DEV];              // the attribute is per device
    std::atomic<bool> &set = attr_set[cur_device()];
    if (!set.load(std::memory_order_relaxed)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_part<PART_WG, BIN_MAX, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BIN_MAX * 12u));
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_part<PART_WG, BIN_MAX, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BIN_MAX * 16u));
        set.store(true, std::memory_order_relaxed);
    }
    if (part_uses_lines(a.n_bins, p64, lines_ok)) {
        const size_t lds_lines = part_lines_lds(a.n_bins, p64);
        if (p64) hipLaunchKernelGGL(k_part_lines<true>, dim3(n_prod), dim3(PART_WG), lds_lines, st, a, binbase, out);
        else     hipLaunchKernelGGL(k_part_lines<false>, dim3(n_prod), dim3(PART_WG), lds_lines, st, a, binbase, out);
        return;
    }
    if (p64) hipLaunchKernelGGL((k_part<PART_WG, BIN_MAX, true>), dim3(n_prod), dim3(PART_WG), (size_t)a.n_bins * 16u, st, a, binbase, out);
    else     hipLaunchKernelGGL((k_part<PART_WG, BIN_MAX, false>), dim3(n_prod), dim3(PART_WG), (size_t)a.n_bins * 12u, st, a, binbase, out);
}

// which of the two first-level kernels launch_part takes on the current device: k_part_lines (true) or k_part (lime_partition_records_dev reports it)
// (defined behind launch_part: the kernels are instantiated in the order of their first use, and this order keeps the code object what it was)
// whole-line writes (k_part_lines) wherever the bins' line buffers fit the LDS next to the stage; LIME_PART_LINES=0: comparison runs
bool part_uses_lines(uint32_t n_bins, bool p64, bool lines_ok)
{
    if (!lines_ok || n_bins > 3u * PART_WG) return false;
    static std::atomic<uint32_t> lines_room[MAX_DEV][2];     // dynamic LDS k_part_lines may ask for on this device (0: not asked yet)
    const size_t lds_lines = part_lines_lds(n_bins, p64);
    const void *kl = p64 ? reinterpret_cast<const void *>(k_part_lines<true>) : reinterpret_cast<const void *>(k_part_lines<false>);
    std::atomic<uint32_t> &room = lines_room[cur_device()][p64 ? 1 : 0];
    uint32_t r = room.load(std::memory_order_relaxed);
    if (!r) {
        hipFuncAttributes fa;
        r = 1u;
        if (hipFuncGetAttributes(&fa, kl) == hipSuccess && fa.sharedSizeBytes < 160u * 1024u) {
            const uint32_t dyn = 160u * 1024u - (uint32_t)fa.sharedSizeBytes;
            if (hipFuncSetAttribute(kl, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) == hipSuccess) r = dyn;
        }
        (void)hipGetLastError();
        room.store(r, std::memory_order_relaxed);
    }
    // two workgroups per CU must fit (the kernel is a chain of short phases: alone on a CU it is slower than k_part -- configs[2], 1193 bins:
    // 0.72 against 0.48 ms; N = 1e10, 477 bins, two per CU: 3.8 against 4.2 .. 4.7 ms)
    const size_t stat = 160u * 1024u - (r > 1u ? r : 0u);               // the kernel's static LDS
    return lds_lines <= r && 2u * (lds_lines + stat + 512u) <= 160u * 1024u;
}

void launch_part2(const uint32_t *recs, const uint64_t *binbase, uint32_t n_bins, uint32_t bin_shift, uint64_t *regbase,
                  uint32_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_part2, dim3(n_bins), dim3(PART_WG), 0, st, recs, binbase, bin_shift, regbase, out);
}

// second level by tiles (k_sort_tiles + k_apply_tiles).  tbase: n_bins + 1 words; idx: (tiles + n_bins) * (f2 + 1) 16-bit entries;
// out16: PART_TILE 16-bit records per tile row (tiles_bound() rows at most)
void launch_sort_tiles(const uint32_t *recs, const uint64_t *binbase, uint32_t n_bins, uint32_t bin_shift, uint32_t *tbase, uint16_t *idx, uint16_t *out16,
                       hipStream_t st, bool big_rows, bool tbase_ready)
{
    if (!tbase_ready) hipLaunchKernelGGL(k_tile_bases, dim3(1), dim3(PART_WG), 0, st, binbase, n_bins, tbase);
    // enough workgroups to fill the device evenly: about 8 per CU (two are resident at a time)
    const uint32_t per_bin = n_bins >= 2048u ? 1u : (2048u + n_bins - 1u) / n_bins;
    hipLaunchKernelGGL(k_sort_tiles, dim3(n_bins, per_bin), dim3(PART_WG), 0, st, recs, binbase, bin_shift, tbase, idx, out16, big_rows ? 1u : 0u);
}

uint64_t tiles_bound(uint64_t n_records, uint32_t n_bins) { return n_records / PART_TILE + n_bins; }

uint32_t part_tile() { return PART_TILE; }
uint32_t row_stride() { return ROW_STRIDE; }

void launch_regroup(const uint32_t *rx, const uint64_t *srcoff, uint32_t n_src, uint32_t nb, const uint64_t *dstbase, uint32_t *dst, hipStream_t st)
{
    if (nb) hipLaunchKernelGGL(k_regroup, dim3(nb), dim3(256), 0, st, rx, srcoff, n_src, nb, dstbase, dst);
}

void preload_partition()
{
    preload_kernel(k_part<PART_WG, BIN_MAX, false>); preload_kernel(k_part<PART_WG, BIN_MAX, true>);
    preload_kernel(k_part_lines<false>); preload_kernel(k_part_lines<true>); preload_kernel(k_tile_bases); preload_kernel(k_sort_tiles);
}

} // namespace lime
