// lime_kernels.hip -- hand-written HIP kernels (gfx950 / CDNA4, wave64) for LiME's hot path:
// alpha-cluster detection over lcp/da (reference: src/ClusterLCP.cpp:140-283) and per-cluster
// read x genome similarity accumulation over ebwt/da (reference: src/ClusterBWT_DA.cpp:256-358).
//
// Design: the unit of work is a POSITION; clusters are segments delimited by
// head(i) := lcp[i] < alpha.  Every WAVE is an independent worker over 1024-position windows (+16
// positions of read-ahead): lane-strided dword loads (register j of lane l = position 64 j + l),
// the next window's loads in flight while the current one is worked on, no workgroup barrier in
// the loop; the waves of a workgroup (one per CU) draw their windows from one LDS counter.  Per
// window: head / read bits as wave ballots (= mask words), acceptance of the segments by carry-ripple
// arithmetic on 16-bit chunks, a list of the accepted clusters' positions in LDS, clusters of 2..4
// symbols one per lane, 5..16 by fixed lane groups, 17..64 one at a time by the whole wave; table
// updates are queued in LDS and leave either as compare-and-swaps on the packed byte cells (exact
// modulo 256 like the reference's unsigned char) or as 4-byte records that later kernels bin and
// apply through LDS.  Segments still open after the read-ahead are closed by k_resolve_open /
// k_resolve; clusters longer than 64 go to a one-workgroup-per-cluster hash kernel.  Integer / byte
// work only: no MFMA, HBM-bound.
//
// This file: the scan and detection kernels, the list and long-cluster scorers, the kernels over the finished table and the small
// utilities.  The partition kernels are in lime_partition.hip, the apply kernels in lime_apply.hip.
#define LIME_DEBUG_TU_SCAN          // lime_debug.h: this file defines the LIME_WALL_TIMING globals
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <type_traits>
#include "lime_device.h"
#include "lime_kernels.h"
#include "lime_wave.h"
#include "lime_debug.h"
#include "lime_launch.h"

namespace lime {

// ---- flag byte kept per staged position -------------------------------------------------
constexpr uint32_t F_SYM = 0x0F;
constexpr uint32_t F_READ = 0x20;
constexpr uint32_t F_GEN = 0x40;

constexpr uint32_t MID_MAX = 64;      // clusters of SMALL_MAX+1 .. MID_MAX symbols: scored by the scan as one 64-lane group each
constexpr uint32_t QCAP = 320;        // pending table updates per wave (a batch of 64 small clusters adds <= 256)
// queue entry: genome | t << T_SHIFT (lime_kernels.h): 7 bits of t; a cluster scored in the scan has <= MID_MAX symbols, so t <= MID_MAX / 2
static_assert(MID_MAX / 2u < (1u << (32u - T_SHIFT)), "the queue's t field must hold the largest in-scan pair score");
constexpr uint32_t CAP_A = 256;       // clusters (2..SMALL_MAX symbols) a window can own
constexpr uint32_t CAP_D = 256;       // of those, clusters with a repeated document (general routine)


// LDS of ONE wave: the staged window and its work lists.  `da`/`fl` are sized by the kernel.
template <uint32_t NPOS>
struct alignas(16) WaveLds {
    uint32_t da[NPOS];
    uint8_t fl[NPOS];
    alignas(8) uint8_t hb[NPOS / 8 + 8];   // head bit of every staged position of the scan, same layout as rb (read as 64-bit words)
    alignas(8) uint8_t rb[NPOS / 8 + 8];   // read bit of every staged position (byte k = positions 8k..8k+7)
    uint16_t listM[WIN / 5 + 4];      // scan: this window's clusters of 5..SMALL_MAX symbols (start | (len-1) << 12)
    uint32_t m_tstart[64];            //       first pair-task of each of them
    uint8_t m_flag[64], m_dup[64];
    alignas(8) uint64_t asw[NW];                 // scan: per mask word, heads of the clusters scored in the window
    uint32_t prew[NW];                 //       and how many such heads the words before hold
    uint16_t listA[CAP_A], listD[CAP_D];   // entry: start | (len-1) << 12
    uint32_t q_read[QCAP], q_gen[QCAP];
};


// threads per workgroup of k_scan and waves per SIMD it is compiled for: ScanCfg in lime_kernels.h (one workgroup per CU:
// EBWT = 0: 16 waves = 4 per SIMD; EBWT = 1: 12 waves = 3 per SIMD); the LDS of one wave is kept small: it bounds them
constexpr uint32_t DUP_SLOTS = 8;     // clusters with a repeated document a wave of k_scan holds before scoring them
constexpr uint32_t DUP_SLOTS_E = 4;   // ... with symbols (EBWT=1: 16 waves per CU, the LDS is short): one flush of four 16-lane groups
// QCAP_SCAN, QCAP_SCAN_SHORT (the update queue / record buffers of a wave): lime_kernels.h


// byte -> symbol index, and symbol index -> set of symbol indices it scores 1 against
// (iupac_match); filled once per workgroup
// pairlut[rmask | (len-1) << 4] for a cluster of len = 2..4 symbols with read bits rmask: bit k = position
// pair k of (0,1)(0,2)(0,3)(1,2)(1,3)(2,3) joins a read with a genome inside the cluster, bit 8+k =
// the pair's FIRST position is the read
// pairs[rmask | (len-1) << 4]: the read x genome pairs of a cluster of len = 2..4 symbols with read bits rmask, as a
// list of up to four slots of 7 bits (read position | genome position << 2 | number of the position pair << 4) and
// their count in bits 28..30
struct WgTables { uint8_t symidx[256]; uint16_t compat[16]; uint16_t pairlut[64]; uint16_t compatb[256]; uint32_t pairs[64]; };   // compatb[byte] = compat[symidx[byte]]

__device__ __forceinline__ void tables_init(WgTables &T)
{
    const uint32_t t = threadIdx.x;
    for (uint32_t b = t; b < 256u; b += blockDim.x) {
        const uint32_t si = sym_index(b);
        uint32_t m = 0;
        for (uint32_t k = 0; k < 16u; ++k) m |= iupac_match(si, k) << k;
        T.symidx[b] = (uint8_t)si; T.compatb[b] = (uint16_t)m;
    }
    if (t < 16u) {
        uint32_t m = 0;
        for (uint32_t b = 0; b < 16u; ++b) m |= iupac_match(t, b) << b;
        T.compat[t] = (uint16_t)m;
    }
    for (uint32_t e = t; e < 64u; e += blockDim.x) {
        const uint32_t len = (e >> 4) + 1u, vm = (1u << len) - 1u, r = e & 15u & vm, g = ~r & vm;
        uint32_t v = 0, k = 0;
        for (uint32_t i = 0; i < 4u; ++i)
            for (uint32_t j = i + 1u; j < 4u; ++j, ++k) {
                const uint32_t ri = (r >> i) & 1u, rj = (r >> j) & 1u, gi = (g >> i) & 1u, gj = (g >> j) & 1u;
                v |= ((ri & gj) | (gi & rj)) << k;
                v |= ri << (8u + k);
            }
        T.pairlut[e] = (uint16_t)v;
        uint32_t pv = 0, np = 0;
        k = 0;
        for (uint32_t i = 0; i < 4u; ++i)
            for (uint32_t j = i + 1u; j < 4u; ++j, ++k) {
                const uint32_t ri = (r >> i) & 1u, rj = (r >> j) & 1u, gi = (g >> i) & 1u, gj = (g >> j) & 1u;
                if ((ri & gj) | (gi & rj)) { pv |= ((ri ? i : j) | ((ri ? j : i) << 2) | (k << 4)) << (7u * np); ++np; }
            }
        T.pairs[e] = pv | (np << 28);
    }
    __syncthreads();
}


// ---- table updates of a wave: queued in its LDS ring, applied together so that the round
// trips of the compare-and-swaps overlap instead of following one another -----------------
struct UpdQueue { uint32_t *qr, *qg; uint32_t n, cap;
    // split-phase mode (k_scan): the compare-and-swaps of a drain are only ISSUED; their results
    // are looked at by the next drain, so a wave never waits for the round trip to the table.
    // Lane l owns in-flight slots 64 j + l (j < 4): entry kept in fr/fg, value the CAS expected
    // and value it returned in registers.
    bool async = false;
    uint32_t *fr = nullptr, *fg = nullptr, *fe = nullptr;   // entry (read, genome | t) and the word value its CAS expected
    uint32_t f_old[4], f_pend = 0;               // f_pend: bit j = slot j occupied, bit 4+j = its word was only LOADED so far
    uint32_t nj = 4;                             // in-flight slots per lane (a constant of the kernel: 4, or 2 where LDS is short)
    // dense tables: once 1 in 4 of the first tries (which expect an empty word) has lost, new entries first load
    // their word (a load is much cheaper than a lost compare-and-swap) and try with what they saw one drain later
    uint32_t f_first = 0, f_lost = 0; bool load_first = false;
    // binned mode (ScanArgs::upd_mode): drains append (cell, t) records to the wave's region of the pool and count
    // them per table bin in the workgroup's LDS histogram; no table access from the scan at all
    bool binned = false; uint32_t *out = nullptr; lds_vu32 *sub_n = nullptr; uint32_t *hist = nullptr;   // out: the wave's n_sub sub-regions; sub_n: records in each (LDS)
    uint32_t *lbuf = nullptr; lds_vu32 *lfill = nullptr;   // one or two sub-regions: finished records wait here (LBUF per sub-region, lfill[s] of them) until they fill 64-byte lines
    // direct mode (round 6; k_scan<.,0,2>: tables of one or two sub-regions): the scorers write FINISHED 4-byte records -- qr[] holds sub-region 0's, qg[]
    // sub-region 1's, n / n1 of them -- and a flush stores their whole 64-byte lines; no queue entry is looked at twice
    bool direct = false;
    uint32_t n1 = 0, base0 = 0, base1 = 0;                 // records waiting in qg[]; records stored so far per sub-region (wave-uniform)
    uint32_t sub_rb = 0xFFFFFFFFu, sub_gb = 0;             // where sub-region 1 begins (read, genome); sub_rb = ~0: one sub-region
    __device__ __forceinline__ bool two() const { return sub_rb != 0xFFFFFFFFu; }
    uint32_t bad = 0;                                      // per lane: a genome index beyond the table was met (LIME_FLAG_DOCID at the next flush / window top)
#ifdef LIME_PHASE_TIMING
    uint64_t t_drain = 0; uint32_t n_drain = 0;
#endif
};

// The scorers that write queue entries or records themselves pass every genome index through genome_ok (lime_device.h, all 32 bits) first:
// the lanes with `hit` are about to store one whose validity is `ok`.  A bad one is noted for report_bad and NOT stored -- no drain, flush or
// partition kernel ever sees a genome index beyond the table (the drains' own tests on the masked index are a second line only).
__device__ __forceinline__ bool checked(UpdQueue &q, bool hit, bool ok) { q.bad |= (uint32_t)(hit && !ok); return hit && ok; }
__device__ __forceinline__ void report_bad(UpdQueue &q, const ScanArgs &a)
{
    if (__ballot(q.bad != 0u)) { if (q.bad) atomicOr(&cold(a).stats->flags, LIME_FLAG_DOCID); q.bad = 0u; }
}

// The wave's region of the record pool (n_sub sub-regions of cap_w records), recomputed where it is needed from the kernel's arguments and the wave's number
__device__ __forceinline__ uint32_t *pool_of(const ScanArgs &ca, uint32_t n_sub, uint32_t cap_w)
{
    const uint32_t wave_gid = blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return ca.pool + (size_t)wave_gid * n_sub * cap_w;
}

// Split-phase drain: (1) settle the slots issued last time: a CAS that found the expected word is
// done, one that lost keeps its slot with the word it saw, a slot that only loaded its word now knows
// what to expect; (2) free slots take entries from the queue's tail; (3) every occupied slot issues
// its CAS (or, for a new entry in load-first mode, the load of its word).  Entries that found no free
// slot stay queued (q.n > 0 afterwards): callers loop while they need more room.
__device__ __forceinline__ void drain_async(UpdQueue &q, const ScanArgs &a)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((uint32_t)j >= q.nj) break;
        const bool pend = (q.f_pend >> j) & 1u, fresh = (q.f_pend >> (4 + j)) & 1u;
        const uint32_t e = pend ? q.fe[64u * (uint32_t)j + lane] : 0u;
        const bool tried = pend && !fresh, lost = tried && q.f_old[j] != e;
        if (j == 0 && !q.load_first) {                     // statistics of the "expect an empty word" first tries (slot 0 as a sample)
            const uint64_t mf = __ballot(tried && e == 0u);
            q.f_first += (uint32_t)__popcll(mf); q.f_lost += (uint32_t)__popcll(mf & __ballot(lost));
        }
        if (tried && !lost) q.f_pend &= ~(1u << j);
        if (fresh || lost) { q.fe[64u * (uint32_t)j + lane] = q.f_old[j]; q.f_pend &= ~(16u << j); }
    }
    if (!q.load_first && q.f_first >= 64u && 4u * q.f_lost >= q.f_first) q.load_first = true;
    uint32_t n = q.n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((uint32_t)j >= q.nj) break;
        const bool fre = !((q.f_pend >> j) & 1u);
        const uint64_t m = __ballot(fre);
        const uint32_t r = (uint32_t)__popcll(m & lt), c = (uint32_t)__popcll(m);
        if (fre && r < n) {
            const uint32_t k = n - 1u - r;
            const uint32_t gt = q.qg[k];
            if ((gt & ((1u << T_SHIFT) - 1u)) >= a.n_refs) atomicOr(&cold(a).stats->flags, LIME_FLAG_DOCID);   // (a second line, like drain_bin's: the writers of the entries test the whole index)
            else {
                q.fr[64u * (uint32_t)j + lane] = q.qr[k]; q.fg[64u * (uint32_t)j + lane] = gt;
                q.fe[64u * (uint32_t)j + lane] = 0u;
                q.f_pend |= (q.load_first ? 17u : 1u) << j;
            }
        }
        n -= c < n ? c : n;
    }
    q.n = n;
    if (ABL(5)) { q.f_pend = 0; return; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((uint32_t)j < q.nj && ((q.f_pend >> j) & 1u)) {
            const uint32_t gt = q.fg[64u * (uint32_t)j + lane];
            const uint64_t cell = (uint64_t)q.fr[64u * (uint32_t)j + lane] * a.n_refs + (gt & ((1u << T_SHIFT) - 1u));
            uint32_t *w = reinterpret_cast<uint32_t *>(a.sim + (cell & ~3ull));
            if ((q.f_pend >> (4 + j)) & 1u) {
                q.f_old[j] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // device-coherent: not a stale L2 line
            } else {
                const uint32_t sh = (uint32_t)(cell & 3ull) * 8u, e = q.fe[64u * (uint32_t)j + lane];
                const uint32_t b = ((e >> sh) + (gt >> T_SHIFT)) & 255u;
                q.f_old[j] = atomicCAS(w, e, (e & ~(255u << sh)) | (b << sh));
            }
        }
}

// Tables of one or two sub-regions (up to 8 GB): the queue's entries become finished 4-byte records in a small LDS
// buffer per sub-region, and only WHOLE 64-byte lines leave it (partial-line writes cost the N = 10^10 scan 5 %); up to 15
// records per sub-region wait there for the next drain, as records -- nothing is looked at twice (the first version
// kept them as queue entries: a counting loop, a compaction of the kept entries and their 64-bit cell arithmetic again in
// every drain, ~200 vector instructions per window).  `final`: the kernel's last drain writes the partial lines too.
constexpr uint32_t LBUF = 80;                                     // <= 15 waiting + 64 new records per sub-region
__device__ __forceinline__ void drain_lines(UpdQueue &q, const ScanArgs &a, bool final)
{
    const uint32_t lane = lane_id();
    const uint32_t n = q.n;
    const ScanArgs &ca = cold(a);                                 // the fields a drain needs are loaded here, not held through the window loop
    const uint32_t cap_w = ca.cap_w, bin_shift = ca.bin_shift, sub_rb = ca.sub_rb, sub_gb = ca.sub_gb, n_refs = ca.n_refs;
    uint32_t f0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.lfill[0]), f1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.lfill[1]);
    const uint32_t hoff = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.sub_n[MAX_SUB]);
    auto flush = [&](uint32_t sub, uint32_t &f, uint32_t keep_mask) {      // keep_mask = 15: whole lines only; 0: everything
        const uint32_t nl = f & ~keep_mask;
        if (!nl) return;
        const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.sub_n[sub]);
        uint32_t *lb = q.lbuf + sub * LBUF;
        const uint32_t rec = lb[lane < nl ? lane : 0u];
        const uint32_t slot = base + lane;
        if (lane < nl && slot < cap_w && !ABL(7)) {               // a full sub-region only counts (sub_n): the pass is repeated with a larger pool
            const uint32_t bin = rec_bin(rec, sub, bin_shift);
            atomicAdd(&q.hist[hoff + bin], 1u);                   // the histogram counts exactly the records that are stored
            if (!ABL(6)) __builtin_nontemporal_store(rec, q.out + (size_t)sub * cap_w + slot);
        }
        const uint32_t rem = f - nl;
        const uint32_t mv = lb[lane < rem ? nl + lane : 0u];      // (all lanes read before any writes: one instruction each)
        if (lane < rem) lb[lane] = mv;
        if (lane == 0) q.sub_n[sub] = base + nl;
        f = rem;
    };
    for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const bool on = k < n;
        const uint32_t gt = q.qg[on ? k : 0u], rd = q.qr[on ? k : 0u];
        const uint32_t g = gt & (MAX_REFS - 1u);
        // (a second line: every writer of queue entries passes its genome index through genome_ok first, so no entry beyond the
        // table gets here; one that did would be dropped and the pass fail with LIME_ERR_DOCID)
        const bool bad = on && g >= n_refs;
        if (__ballot(bad)) { if (bad) atomicOr(&cold(a).stats->flags, LIME_FLAG_DOCID); }
        const uint32_t rec = rec_of(rd, g, n_refs);               // the cell's low 32 bits
        const bool hi = rec_sub2(rd, g, sub_rb, sub_gb) != 0u;
        uint32_t left = (on && !bad) ? gt >> T_SHIFT : 0u;
        while (__ballot(left != 0u)) {                            // once, unless a pair scored more than 1
            const bool act = left != 0u;
            const uint64_t m1 = __ballot(act && hi), m0 = __ballot(act && !hi);
            if (act) q.lbuf[hi ? LBUF + f1 + rank_in(m1) : f0 + rank_in(m0)] = rec;
            f0 += (uint32_t)__popcll(m0); f1 += (uint32_t)__popcll(m1);
            left -= (uint32_t)act;
            flush(0u, f0, 15u);
            if (m1) flush(1u, f1, 15u);
        }
    }
    q.n = 0;
    if (final) { flush(0u, f0, 0u); flush(1u, f1, 0u); }
    if (lane == 0) { q.lfill[0] = f0; q.lfill[1] = f1; }
}

// Direct mode (round 6).  Ablation cuts showed what the queue -> record -> line-buffer copy of drain_lines costs beyond its stores: 223 of 1586 us on
// configs[2], 2.3 of 14.7 ms at N = 1e10, 61 of 251 us on the text workload (profiles/r06_scan_cuts.txt: the scan without ANY drain work runs at the
// memory floor, 1234 us) -- two LDS reads per entry, a quarter-rate multiply, two ballots and ranks, an LDS write, then the line buffer's read-back, and
// all of it in front of the next window's loads.  Here the scorers compute the record themselves (one multiply-add where they used to write two words)
// and write it where its 64-byte line is being gathered; what is left for the flush is: read 64 records, count them in the bin histogram, store.
//
// A flush stores the LAST nl records waiting in a sub-region's buffer, buf[n - nl .. n), and the front stays where it is (the order of a wave's
// records is free: drain_bin takes the queue's last 64 for the same reason) -- until round 7 it stored the first nl and moved the <= 15 behind them
// to the front, an LDS read, a wait and an LDS write per sub-region and window in front of the next window's loads.  How many leave (`why`):
//   FLUSH_ROOM   a scorer needs room: every whole line, nl = n & ~15, so at most 15 records stay -- the loops `while (n + batch > cap) flush` of
//                put_rec, score_small3 and drain() end after ONE call because of that (static_asserts below), and only this form is reachable from them;
//   FLUSH_TOP    the window's top: whole groups of ScanArgs::flush_gran records (64: every iteration runs with all lanes and every store instruction
//                writes four whole lines; a sub-region with fewer waiting is skipped this window -- up to 63 stay; 16: as FLUSH_ROOM; 0, the default:
//                64 for a table of two sub-regions, whose second one gets a trickle of records that fills a batch every few windows -- configs[2]:
//                scan 1.49 -> 1.46 ms --, 16 for one sub-region, where batches of 64 measured 0.8 % SLOWER at N = 1e10: profiles/r07_flush_ab.txt);
//   FLUSH_FINAL  the kernel's end: everything, the partial line too.
// base0 / base1 advance by multiples of 16 except in the final flush, so every store before it is a whole 64-byte line of the pool.
enum FlushWhy { FLUSH_ROOM = 0, FLUSH_TOP = 1, FLUSH_FINAL = 2 };
static_assert(ROOM_LEFT + 256u <= QCAP_SCAN, "EBWT=0: a whole batch of score_small3 (64 clusters x 4 pairs) fits behind what a room flush leaves");
static_assert(ROOM_LEFT + 128u <= QCAP_SCAN_SHORT, "EBWT=1: half a batch of score_small3 (64 clusters x 2 pair slots) fits behind what a room flush leaves");
static_assert(256u + 2u * ROOM_LEFT <= QCAP_SCAN, "EBWT=0: score_small3's `halves` rule never splits a batch of the long queue");
static_assert(ROOM_LEFT + 64u <= QCAP_SCAN_SHORT && ROOM_LEFT + 64u <= QCAP_SCAN, "a put_rec (<= 64 records) fits behind what a room flush leaves");
// the kernel arguments a flush reads: loaded where it is called, or -- the window's top -- ahead of it
struct FlushK { uint32_t cap_w, bin_shift, n_sub, n_bins, prod_waves, flush_gran; uint32_t *pool; };
__device__ __forceinline__ FlushK flush_args(const ScanArgs &a)
{
    const ScanArgs &ca = cold(a);
    return FlushK{ca.cap_w, ca.bin_shift, ca.n_sub, ca.n_bins, ca.prod_waves, ca.flush_gran, ca.pool};
}
__device__ __forceinline__ void flush_direct(UpdQueue &q, const ScanArgs &a, FlushWhy why, const FlushK &ca)
{
    if (ABL(13)) return;
    if (ABL(14)) { q.n = 0; q.n1 = 0; return; }                      // (timing experiments: the scorers' share of the record work without the flush)
    const uint32_t lane = lane_id();
    const uint32_t cap_w = ca.cap_w, bin_shift = ca.bin_shift, n_sub = ca.n_sub, bin_lim = ca.n_bins;
    const uint32_t hoff = ((uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) / ca.prod_waves) * bin_lim;     // the producer group's part of the workgroup's histogram
    // records that may stay: a compile-time constant except at the window's top (flush_gran is 0, 16 or 64: lime_set_option)
    const bool batches = ca.flush_gran ? ca.flush_gran == FLUSH_GRAN : n_sub == 2u;
    const uint32_t keep = why == FLUSH_FINAL ? 0u : why == FLUSH_TOP && batches ? FLUSH_GRAN - 1u : ROOM_LEFT;
    report_bad(q, a);
    const uint32_t wave_gid = blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *const out = ca.pool + (size_t)wave_gid * n_sub * cap_w;      // the wave's region of the pool (pool_of)
#pragma unroll
    for (uint32_t sub = 0; sub < 2u; ++sub) {
        if (sub && !q.two()) break;
        const uint32_t n = sub ? q.n1 : q.n, nl = n & ~keep;
        if (!nl) continue;                                           // wave-uniform
        const uint32_t *buf = (sub ? q.qg : q.qr) + (n - nl);        // the last nl records
        const uint32_t base = sub ? q.base1 : q.base0;
        for (uint32_t k0 = 0; k0 < nl; k0 += 64u) {
            const uint32_t k = k0 + lane;
            const bool on = k < nl;
            const uint32_t rec = buf[on ? k : 0u], slot = base + k;
            uint32_t bin = rec_bin(rec, sub, bin_shift);
            bin = bin < bin_lim ? bin : bin_lim - 1u;                // (a second line: the scorers store no record of a cell beyond the table)
            if (on && slot < cap_w && !ABL(7)) {                     // a full sub-region only counts: the pass is repeated with a larger pool
                atomicAdd(&q.hist[hoff + bin], 1u);                  // the histogram counts exactly the records that are stored
                if (!ABL(6)) __builtin_nontemporal_store(rec, out + (size_t)sub * cap_w + slot);
            }
        }
        if (sub) { q.base1 = base + nl; q.n1 = n - nl; } else { q.base0 = base + nl; q.n = n - nl; }
    }
}
__device__ __forceinline__ void flush_direct(UpdQueue &q, const ScanArgs &a, FlushWhy why) { flush_direct(q, a, why, flush_args(a)); }

// direct mode: the lanes with `hit` append the record of (read rd, genome index gd), t = 1.  All 64 lanes call.
// The callers have taken the lanes whose gd fails genome_ok out of `hit` (checked()): every record stored is a cell of the table.
__device__ __forceinline__ void put_rec(UpdQueue &q, const ScanArgs &a, bool hit, uint32_t rd, uint32_t gd)
{
    if (ABL(13)) return;
    const uint32_t rec = rec_of(rd, gd, a.n_refs);                   // the cell's low 32 bits
    if (!q.two()) {
        const uint64_t m = __ballot(hit);
        const uint32_t tot = (uint32_t)__popcll(m);
        // ends after one call: a room flush leaves q.n <= ROOM_LEFT and tot <= 64, ROOM_LEFT + 64 <= q.cap (static_assert above)
        while (q.n + tot > q.cap) flush_direct(q, a, FLUSH_ROOM);
        if (hit) q.qr[q.n + rank_in(m)] = rec;
        q.n += tot;
    } else {
        const bool hi = rec_sub2(rd, gd, q.sub_rb, q.sub_gb) != 0u;               // cell >= 2^32
        const uint64_t m1 = __ballot(hit && hi), m0 = __ballot(hit && !hi);
        const uint32_t t0 = (uint32_t)__popcll(m0), t1 = (uint32_t)__popcll(m1);
        // ends after one call: a room flush leaves q.n and q.n1 <= ROOM_LEFT, and t0 + t1 <= 64
        while (q.n + t0 > q.cap || q.n1 + t1 > q.cap) flush_direct(q, a, FLUSH_ROOM);
        if (hit) { if (hi) q.qg[q.n1 + rank_in(m1)] = rec; else q.qr[q.n + rank_in(m0)] = rec; }
        q.n += t0; q.n1 += t1;
    }
}

// Binned mode: the queue's entries become 4-byte pool records in the wave's own region: the LOW 32 bits of the cell; the
// high part picks one of the wave's n_sub sub-regions and the score is implicit (a pair that scores t > 1 -- repeated
// documents only -- leaves t records).  Every byte the scan stores costs its read stream dearly -- a gigabyte of appended
// records slows 8 GB of loads from 1.15 to 1.76 ms whatever the layout of the stores (tools/load_bench.hip) -- so the
// records are as short as they can be.  Records beyond a sub-region's capacity are only counted (the host repeats the pass
// with a larger pool: LIME_FLAG_POOL_FULL).  One or two sub-regions (tables up to 8 GB): drain_lines above; more: here,
// 64 records at a time as they come.
// `whole`: every entry leaves (the window's top, the kernel's end); else -- a scorer needs room in the middle of a window -- only the LAST 64: a full
// batch (the order of the records is free), instead of a full one and the few entries behind it every time.
__device__ __forceinline__ void drain_bin(UpdQueue &q, const ScanArgs &a, bool final = false, bool whole = true)
{
    if (cold(a).n_sub <= 2u) { drain_lines(q, a, final); return; }         // (re-read: a flag held through the window loop is a pair of SGPRs)
    // Three and more sub-regions.  Until round 6 the records of such a table left "as they came": every 64 queue entries split three to eight ways by a
    // loop over the sub-regions (a ballot, a rank, an LDS read and write of the sub-region's count each), so nearly every store was a part of a
    // 64-byte line -- the stores alone were 2.65 of the 16.7 ms of the scan at configs[4]'s shape, and where records are dense the loop was a third of
    // the scan (5.3 of 20.7 ms on the clustered generator; profiles/r06_scan_cuts.txt).  Now there is no loop: a lane takes its record's place in its
    // sub-region with ONE LDS atomic on the sub-region's running count (sub_n[]: the hardware serialises the lanes of one address), and only whole
    // lines leave: a record whose place lies in a line that this batch completes is stored from its register, the others wait in LDS (lbuf[16 s + i]:
    // record i of sub-region s's open line), and the records that waited in a line completed now are stored by the lanes 16 s + i that read them
    // back at the top (two store instructions into one line, back to back: they meet in L2).  The order of a sub-region's records is whatever the
    // LDS made it -- the table is a sum.
    const uint32_t lane = lane_id();
    const ScanArgs &ca = cold(a);
    const uint32_t n = q.n, n_sub = ca.n_sub, cap_w = ca.cap_w, n_refs = ca.n_refs, bin_shift = ca.bin_shift;
    const uint32_t hoff = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.sub_n[MAX_SUB]);
    uint32_t *const out = pool_of(ca, n_sub, cap_w);
    const uint32_t ws = lane >> 4, wi = lane & 15u;               // this lane's part in storing waiting records: record wi of sub-region ws (and ws + 4)
    // the waiting records of sub-regions ws / ws + 4 whose line the batch completed (counts c0 before, c1 after) leave
    auto store_waiting = [&](uint32_t sub, uint32_t c0, uint32_t c1, uint32_t wrec) {
        const uint32_t l0 = c0 & ~15u;
        if (sub < n_sub && (c1 & ~15u) != l0 && wi < (c0 & 15u) && l0 + wi < cap_w && !ABL(7)) {     // a full sub-region only counts: the pass is repeated with a larger pool
            atomicAdd(&q.hist[hoff + rec_bin(wrec, sub, bin_shift)], 1u);      // the histogram counts exactly the records that are stored
            if (!ABL(6)) out[(size_t)sub * cap_w + l0 + wi] = wrec;       // (a plain store, like the other piece of its line below: a non-temporal store of less than a line is a read-modify-write at the memory, 4.5 x a whole line's -- plain, the two pieces meet in L2)
        }
    };
    const uint32_t first = whole || n <= 64u ? 0u : n - 64u;      // entries [first, n) leave
    for (uint32_t k0 = first; k0 < n; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const bool on = k < n;
        const uint32_t gt = q.qg[on ? k : 0u], rd = q.qr[on ? k : 0u];
        // (a second line: every writer of queue entries passes its genome index through genome_ok first, so no entry beyond the
        // table gets here; one that did would be dropped and the pass fail with LIME_ERR_DOCID)
        const uint64_t cell = cell_of(rd, gt & (MAX_REFS - 1u), n_refs);
        const uint32_t hi = cell_sub(cell), rec = (uint32_t)cell;
        const bool bad = on && ((gt & (MAX_REFS - 1u)) >= n_refs || hi >= n_sub);
        if (__ballot(bad)) { if (bad) atomicOr(&cold(a).stats->flags, LIME_FLAG_DOCID); }
        uint32_t left = (on && !bad) ? gt >> T_SHIFT : 0u;
        while (__ballot(left != 0u)) {                            // once, unless a pair scored more than 1
            const bool act = left != 0u;
            const uint32_t wv0 = q.lbuf[lane], c00 = q.sub_n[ws];
            uint32_t wv1 = 0, c04 = 0;
            if (n_sub > 4u) { wv1 = q.lbuf[64u + lane]; c04 = q.sub_n[4u + ws]; }                   // wave-uniform
            uint32_t slot = 0;
            if (act) slot = __hip_atomic_fetch_add(&q.sub_n[hi], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t c1h = q.sub_n[act ? hi : 0u], c10 = q.sub_n[ws];
            const uint32_t lim = c1h & ~15u;                      // the whole lines of this lane's sub-region end here
            if (act) {
                if (slot >= lim) q.lbuf[16u * hi + (slot & 15u)] = rec;
                else if (slot < cap_w && !ABL(7)) {
                    atomicAdd(&q.hist[hoff + cell_bin(cell, bin_shift)], 1u);
                    if (!ABL(6)) out[(size_t)hi * cap_w + slot] = rec;
                }
            }
            store_waiting(ws, c00, c10, wv0);
            if (n_sub > 4u) store_waiting(4u + ws, c04, q.sub_n[4u + ws], wv1);
            left -= (uint32_t)act;
        }
    }
    q.n = first;
    if (final) {                                                  // the kernel's last drain: the open lines too (c1 = c0 + 16: "completed")
        const uint32_t c00 = q.sub_n[ws], wv0 = q.lbuf[lane];
        store_waiting(ws, c00, c00 + 16u, wv0);
        if (n_sub > 4u) { const uint32_t c04 = q.sub_n[4u + ws], wv1 = q.lbuf[64u + lane]; store_waiting(4u + ws, c04, c04 + 16u, wv1); }
    }
}
__device__ __forceinline__ void drain(UpdQueue &q, const ScanArgs &a)
{
    if (ABL(13)) { q.n = 0; q.n1 = 0; return; }            // (timing experiments: what ALL of the drains' work costs -- the entries are thrown away)
    if (q.direct) { flush_direct(q, a, FLUSH_ROOM); return; }          // (a scorer's `while (no room) drain`: never the window top's form, which may leave 63)
    if (q.async) { if (q.binned) drain_bin(q, a, false, false); else drain_async(q, a); return; }     // both flags are compile-time constants of the kernel
#ifdef LIME_PHASE_TIMING
    const uint64_t t0 = __builtin_readcyclecounter();
#endif
    // four queue entries per lane and round: their compare-and-swaps are issued together (first
    // try: word still zero, tables are sparse) and only the ones that lost are tried again
    if (!ABL(5))
        for (uint32_t k0 = 0; k0 < q.n; k0 += 256u) {
            uint32_t *w[4], sh[4], t[4], expect[4], pend = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t k = k0 + 64u * (uint32_t)j + lane_id();
                const bool on = k < q.n;
                const uint32_t gt = q.qg[on ? k : 0u];
                const uint64_t cell = (uint64_t)q.qr[on ? k : 0u] * a.n_refs + (gt & ((1u << T_SHIFT) - 1u));
                w[j] = reinterpret_cast<uint32_t *>(a.sim + (cell & ~3ull));
                sh[j] = (uint32_t)(cell & 3ull) * 8u; t[j] = gt >> T_SHIFT; expect[j] = 0u;
                pend |= (uint32_t)on << j;
            }
            while (__ballot(pend != 0u)) {
                uint32_t old[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((pend >> j) & 1u) {
                        const uint32_t b = ((expect[j] >> sh[j]) + t[j]) & 255u;
                        old[j] = atomicCAS(w[j], expect[j], (expect[j] & ~(255u << sh[j])) | (b << sh[j]));
                    }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((pend >> j) & 1u) {
                        if (old[j] == expect[j]) pend &= ~(1u << j);
                        else expect[j] = old[j];
                    }
            }
        }
    q.n = 0;
#ifdef LIME_PHASE_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    q.t_drain += __builtin_readcyclecounter() - t0; ++q.n_drain;
#endif
}

// every active lane may add one update; all 64 lanes must call (wave ballots inside)
__device__ __forceinline__ uint32_t emit(UpdQueue &q, const ScanArgs &a, bool on, uint32_t rdoc, uint32_t gdoc, uint32_t t)
{
    if (!q.direct) while (q.n + 64u > q.cap) drain(q, a);
    const uint32_t g = gdoc - a.n_reads;
    const bool bad = on && (!genome_ok(g, a.n_refs) || rdoc >= a.n_reads);
    if (__ballot(bad)) { if (bad) atomicOr(&cold(a).stats->flags, LIME_FLAG_DOCID); }
    on = on && !bad;
    if (q.direct) {                                        // a score of t = t records (t > 1: repeated documents only)
        uint32_t left = on ? t : 0u;
        while (__ballot(left != 0u)) { put_rec(q, a, left != 0u, rdoc, g); left -= (uint32_t)(left != 0u); }
        return on ? 1u : 0u;
    }
    const uint64_t m = __ballot(on);
    if (on) {
        const uint32_t slot = q.n + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
        q.qr[slot] = rdoc; q.qg[slot] = g | (t << T_SHIFT);
    }
    q.n += (uint32_t)__popcll(m);
    return on ? 1u : 0u;
}

// ---- general score of short clusters by lane groups ------------------------------------------
// G lanes per cluster, element i on sub-lane i; XOR-ing the sub-lane with 1..R (R + 1 = the power
// of two covering the longest cluster of the wave) shows every lane every other element of its
// cluster.  Pass 1: is this element the first of its document, and the document's count / 16-bin
// histogram over the cluster (counts <= 64: no wrap, no saturation).  Pass 2: every
// first-occurrence read meets every first-occurrence genome once (pair_score;
// ClusterBWT_DA.cpp:107-190 / :192-252).
// the clusters of one wave iteration: element `sub` of the lane's group holds document d and ebwt
// byte bb (sub < len; len = 0: no cluster in this group)
template <int EBWT, int G>
__device__ __forceinline__ uint32_t group_score(const ScanArgs &a, const WgTables &T, UpdQueue &qu,
                                                uint32_t d, uint32_t bb, uint32_t len)
{
    const uint32_t sub = lane_id() & (G - 1u);
    uint32_t acc_upd = 0;
    // rounds: sub-lane ^ r stays inside the first R+1 sub-lanes, which hold the whole cluster
    uint32_t R = 1u;
#pragma unroll
    for (uint32_t p2 = 2u; p2 < (uint32_t)G; p2 <<= 1) if (__ballot(len > p2)) R = 2u * p2 - 1u;
    const bool have = sub < len;
    const uint32_t sy = (EBWT && have) ? T.symidx[bb] : 0u;
    const bool isr = have && d < a.n_reads;
    const uint32_t f = have ? (sy | (isr ? F_READ : F_GEN)) : 0u;
    uint32_t earlier = 0, cnt = have ? 1u : 0u, hs[4] = {0u, 0u, 0u, 0u};
    if (EBWT) hist_add(hs, sy, (uint32_t)have);
#pragma unroll 1
    for (uint32_t r = 1; r <= R; ++r) {
        const uint32_t pd = __shfl_xor(d, (int)r), pf = __shfl_xor(f, (int)r);
        const uint32_t same = (uint32_t)(f && pf && pd == d);
        earlier |= same & (uint32_t)((sub ^ r) < sub);
        cnt += same;
        if (EBWT) hist_add(hs, pf & F_SYM, same);
    }
    const uint32_t lead = (uint32_t)(have && !earlier);
#pragma unroll 1
    for (uint32_t r = 1; r <= R; ++r) {
        const uint32_t pd = __shfl_xor(d, (int)r), pf = __shfl_xor(f, (int)r), pl = __shfl_xor(lead, (int)r), pc = __shfl_xor(cnt, (int)r);
        uint32_t ph[4] = {0u, 0u, 0u, 0u};
        if (EBWT) { ph[0] = __shfl_xor(hs[0], (int)r); ph[1] = __shfl_xor(hs[1], (int)r); ph[2] = __shfl_xor(hs[2], (int)r); ph[3] = __shfl_xor(hs[3], (int)r); }
        const bool pair = lead && isr && pl && (pf & F_GEN);
        if (__ballot(pair) == 0ull) continue;
        uint32_t t = cnt < pc ? cnt : pc;
        if (EBWT) {
            uint32_t h2[4], p2[4];           // only real pairs go through the (possibly slow) score
#pragma unroll
            for (int k = 0; k < 4; ++k) { h2[k] = pair ? hs[k] : 0u; p2[k] = pair ? ph[k] : 0u; }
            t = pair_score(h2, p2);
        }
        acc_upd += emit(qu, a, pair && t, d, pd, t);
    }
    return acc_upd;
}


// ---- clusters with a repeated document, kept by the wave that found them: copies of up to
// DUP_SLOTS clusters (<= SMALL_MAX elements each) in LDS, scored four at a time by 16-lane groups
// when enough have gathered (and at the end).  A full store is scored on the spot, so no cluster
// ever leaves the wave.
template <int EBWT, typename LDS>
__device__ __forceinline__ uint32_t dup_flush(LDS &L, uint32_t &n_dup, const ScanArgs &a, const WgTables &T, UpdQueue &qu)
{
    const uint32_t lane = lane_id(), grp = lane >> 4, sub = lane & 15u;
    uint32_t nupd = 0;
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < n_dup; c0 += 4u) {
        const uint32_t c = c0 + grp;
        const uint32_t len = c < n_dup ? L.g_len[c] : 0u;
        const uint32_t cc = c < n_dup ? c : 0u;
        nupd += group_score<EBWT, 16>(a, T, qu, L.g_doc[cc][sub], EBWT ? L.g_sym[cc][sub] : 0u, len);
    }
    n_dup = 0;
    return nupd;
}

// lanes with `on` hand over the cluster staged at L.da / L.fl[p .. p+len); returns the table updates of
// the flushes it had to make (per lane, like the scoring routines)
template <int EBWT, typename LDS>
__device__ __forceinline__ uint32_t dup_push(LDS &L, uint32_t &n_dup, const ScanArgs &a, const WgTables &T, UpdQueue &qu,
                                             bool on, uint32_t p, uint32_t len)
{
    uint64_t m = __ballot(on);
    uint32_t nupd = 0;
    while (m) {                                            // wave-uniform; one round unless the store fills up
        if (n_dup == LDS::NDUP) nupd += dup_flush<EBWT>(L, n_dup, a, T, qu);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
        const bool take = on && rank < LDS::NDUP - n_dup;
        if (take) {
            const uint32_t slot = n_dup + rank;
            for (uint32_t k = 0; k < len; ++k) { L.g_doc[slot][k] = L.da[p + k]; if (EBWT) L.g_sym[slot][k] = L.fl[p + k]; }
            L.g_len[slot] = (uint8_t)len;
        }
        const uint64_t mt = __ballot(take);
        n_dup += (uint32_t)__popcll(mt);
        m &= ~mt; on = on && !take;
    }
    return nupd;
}

// ---- cluster scoring ----------------------------------------------------------------------
// One lane per cluster of the list (<= SMALL_MAX symbols, staged at L.da/L.fl[s..s+len)).  The
// cluster's read and genome positions are bit masks cut out of the window's mask bytes; the
// lane walks reads x genomes by popping bits (typically one or two pairs).  With all documents
// distinct -- checked only among documents of the same kind, the only ones that can repeat --
// a pair scores iupac_match of its two symbols (EBWT) or 1; a cluster with a repeated document
// goes to the general list instead.
template <int EBWT, typename LDS>
__device__ __forceinline__ uint32_t cluster_pairs(LDS &L, UpdQueue &qu, const ScanArgs &a, const uint16_t *list,
                                                  uint32_t n, uint32_t k_base, uint32_t &nD)
{
    const uint32_t lane = lane_id();
    const uint32_t k = k_base + lane;
    const bool on = k < n;
    const uint32_t item = list[on ? k : 0u];
    const uint32_t s = item & 0xFFFu, len = on ? (item >> 12) + 1u : 0u;
    const uint32_t kb = s >> 3, lenm = (1u << len) - 1u;
    const uint32_t rbits = (uint32_t)L.rb[kb] | ((uint32_t)L.rb[kb + 1u] << 8) | ((uint32_t)L.rb[kb + 2u] << 16);
    const uint32_t rmask = (rbits >> (s & 7u)) & lenm, gmask = ~rmask & lenm;
    // repeated document?  (reads among reads, genomes among genomes)
    uint32_t dup = 0;
#pragma unroll 1
    for (int kind = 0; kind < 2; ++kind) {
        uint32_t mi = kind ? gmask : rmask;
        while (__ballot((mi & (mi - 1u)) != 0u)) {
            const uint32_t rest = mi & (mi - 1u);
            const uint32_t di = L.da[s + (rest ? (uint32_t)__builtin_ctz(mi) : 0u)];
            uint32_t mj = rest;
            while (__ballot(mj != 0u)) {
                const bool actj = mj != 0u;
                const uint32_t dj = L.da[s + (actj ? (uint32_t)__builtin_ctz(mj) : 0u)];
                dup |= (uint32_t)(actj && dj == di);
                mj &= mj - 1u;
            }
            mi = rest;
        }
    }
    const uint64_t dm = __ballot(dup != 0u);
    if (dup) L.listD[nD + (uint32_t)__popcll(dm & ((1ull << lane) - 1ull))] = (uint16_t)item;
    nD += (uint32_t)__popcll(dm);
    uint32_t nupd = 0;
    uint32_t mr = dup ? 0u : rmask;
    while (__ballot(mr != 0u)) {
        const bool actr = mr != 0u;
        const uint32_t i = actr ? (uint32_t)__builtin_ctz(mr) : 0u;
        mr &= mr - 1u;
        const uint32_t rdoc = L.da[s + i], rsym = L.fl[s + i] & F_SYM;
        uint32_t mg = actr ? gmask : 0u;
        while (__ballot(mg != 0u)) {
            const bool actg = mg != 0u;
            const uint32_t j = actg ? (uint32_t)__builtin_ctz(mg) : 0u;
            mg &= mg - 1u;
            const uint32_t gdoc = L.da[s + j];
            const uint32_t t = EBWT ? iupac_match(rsym, L.fl[s + j] & F_SYM) : 1u;
            nupd += emit(qu, a, actg && t, rdoc, gdoc, 1u);
        }
    }
    return nupd;
}

// General routine, one lane per cluster [s, s+len) staged in LDS (len <= SMALL_MAX), any mix of
// repeated documents.  For every read (first occurrence) and every genome (first occurrence)
// the counts / 16-bin histograms are rebuilt by walking the cluster.  Quadratic, rare.
template <int EBWT>
__device__ __forceinline__ uint32_t cluster_general(const uint32_t *da, const uint8_t *fl, UpdQueue &qu, const ScanArgs &a, bool on, uint32_t s, uint32_t len)
{
    const uint32_t e = on ? s + len : s;
    uint32_t nupd = 0;
    for (uint32_t p = s; __ballot(p < e); ++p) {
        const bool pon = p < e;
        const uint32_t fp = pon ? fl[p] : 0u;
        const bool isr = pon && (fp & F_READ);
        const uint32_t rdoc = isr ? da[p] : 0u;
        uint32_t earlier = 0, rcount = 0;
        uint32_t cr[4] = {0u, 0u, 0u, 0u};
        if (isr)
            for (uint32_t q = s; q < e; ++q) {
                const uint32_t same = (da[q] == rdoc);
                rcount += same;
                earlier |= same & (uint32_t)(q < p);
                if (EBWT) hist_add(cr, fl[q] & F_SYM, same);
            }
        const bool rlead = isr && !earlier;
        for (uint32_t q = s; __ballot(rlead && q < e); ++q) {
            const bool qon = rlead && q < e;
            const uint32_t fq = qon ? fl[q] : 0u;
            const bool isg = qon && (fq & F_GEN);
            const uint32_t gdoc = isg ? da[q] : 0u;
            uint32_t gearlier = 0, gcount = 0;
            uint32_t cg[4] = {0u, 0u, 0u, 0u};
            if (isg)
                for (uint32_t x = s; x < e; ++x) {
                    const uint32_t same = (da[x] == gdoc);
                    gcount += same;
                    gearlier |= same & (uint32_t)(x < q);
                    if (EBWT) hist_add(cg, fl[x] & F_SYM, same);
                }
            uint32_t t = 0;
            if (isg && !gearlier) t = EBWT ? pair_score(cr, cg) : (rcount < gcount ? rcount : gcount);
            nupd += emit(qu, a, t != 0u, rdoc, gdoc, t);          // counts <= SMALL_MAX: no wrap, no saturation
        }
    }
    return nupd;
}

// all clusters filed in the wave's list; returns the number of table cells incremented (per lane)
template <int EBWT, typename LDS>
__device__ __forceinline__ uint32_t score_lists(LDS &L, UpdQueue &qu, const ScanArgs &a, uint32_t nA)
{
    uint32_t nupd = 0, nD = 0;
    for (uint32_t k0 = 0; k0 < nA; k0 += 64u) nupd += cluster_pairs<EBWT>(L, qu, a, L.listA, nA, k0, nD);
    for (uint32_t k0 = 0; k0 < nD; k0 += 64u) {
        const uint32_t k = k0 + lane_id();
        const uint32_t item = L.listD[k < nD ? k : 0u];
        nupd += cluster_general<EBWT>(L.da, L.fl, qu, a, k < nD, item & 0xFFFu, (item >> 12) + 1u);
    }
    drain(qu, a);
    return nupd;
}

// Clusters of exactly 2 symbols, one lane per cluster: an accepted one holds one read and one genome (never a repeated document), so it is ONE
// pair -- two documents, the roles by one compare, one compatibility lookup, at most one queue entry per lane (slots from a ballot, no prefix sum).
// Real collections are mostly such clusters (98 % in the text-derived fixture, ~245 per window): a dense window lists them apart from the others
// when it builds its cluster list (round 6: the heads of 2-symbol clusters are bit arithmetic on the chunk's head mask), so a round of them reads
// 64 positions and scores them -- no length from the staged head bits, no filing of the other clusters in between.
// (Rounds 3-5 found them inside the rounds over ALL clusters: list entry, 32 head bits, length, classification, then this routine with its read
// bit from the staged mask: ~140 vector instructions and 11 LDS instructions a round of 64, five rounds a window of text -- half that scan.
// Scoring them where they lie instead -- mask word by mask word, position 64 j + l on lane l, documents by a conflict-free ds_read2 -- was built
// and measured in round 6 and is SLOWER: 16 words a window at 24 % of the lanes cost more LDS and vector instructions than 4 full rounds: text
// scan 0.276 -> 0.285-0.307 ms, profiles/r06_inplace_ab.txt.)
template <int EBWT, typename LDS>
__device__ __forceinline__ uint32_t score_len2(LDS &L, const WgTables &T, UpdQueue &qu, const ScanArgs &a, bool on, uint32_t p)
{
    const uint32_t d0 = L.da[p], d1 = L.da[p + 1u];
    const bool r0 = d0 < a.n_reads;                                          // position p is the read; else p + 1 is
    bool hit = on;
    if (EBWT) hit = hit && ((T.compatb[L.fl[p]] >> T.symidx[L.fl[p + 1u]]) & 1u);
    const uint32_t rd = r0 ? d0 : d1, gd = (r0 ? d1 : d0) - a.n_reads;
    hit = checked(qu, hit, genome_ok(gd, a.n_refs));
    if (qu.direct) { put_rec(qu, a, hit, rd, gd); return hit ? 1u : 0u; }
    const uint64_t m = __ballot(hit);
    const uint32_t tot = (uint32_t)__popcll(m);
    while (qu.n + tot > qu.cap) drain(qu, a);
    if (hit) {
        const uint32_t slot = qu.n + rank_in(m);
        qu.qr[slot] = rd; qu.qg[slot] = gd | (1u << T_SHIFT);
    }
    qu.n += tot;
    return hit ? 1u : 0u;
}

// =========================================================================================
// Round 3 back end of the scan: the same results with about a third of the vector instructions.
// (PMC, configs[2], per 1024-position window, round 2: staging 131, chunk acceptance 82, cluster list 159,
// 2-4-symbol round 214, rows 212 vector instructions; the six predicated emission blocks of the 2-4-symbol routine alone
// compiled to 26 each.)
// =========================================================================================

// Clusters of 2..4 symbols, one lane per cluster.  The pairs that join a read with a genome come as a LIST from a
// table indexed by (read bits, length): at most four slots, so the emission is four short blocks with static queue
// offsets instead of six; the documents of a slot are re-read from the staged window by position (a per-lane
// register index would cost a select chain).  Every genome index passes genome_ok before it is stored; where the
// slots come from the prefix sum over `hits`, a bad one's slot takes a stand-in that stays inside the table.  Two equal documents (only documents of one kind can be equal: six plain compares, positions past the
// cluster carry impossible ids) hand the cluster to the wave's repeat store.
template <int EBWT, typename LDS>
__device__ __forceinline__ uint32_t score_small3(LDS &L, const WgTables &T, UpdQueue &qu, uint32_t &n_dup, const ScanArgs &a,
                                                 bool on, uint32_t p, uint32_t len)
{
    const uint32_t rmask = bits_at(L.rb, p) & ((1u << len) - 1u);
    const uint32_t pl = T.pairs[rmask | (((len - 1u) & 3u) << 4)];          // len == 0 (lane off): an entry without pairs
    uint32_t d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = L.da[p + i];
    d[2] = len > 2u ? d[2] : 0xFFFFFFFEu;
    d[3] = len > 3u ? d[3] : 0xFFFFFFFFu;
    const bool dup = on && ((d[0] == d[1]) | (d[0] == d[2]) | (d[0] == d[3]) | (d[1] == d[2]) | (d[1] == d[3]) | (d[2] == d[3]));
    const uint32_t nflush = dup_push<EBWT>(L, n_dup, a, T, qu, dup, p, len);
    const uint32_t np = pl >> 28;
    uint32_t hits = (1u << np) - 1u;                                          // bit e: slot e of the list scores
    if (EBWT) {
        uint32_t sy[4], cs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const uint32_t by = L.fl[p + i]; sy[i] = T.symidx[by]; cs[i] = T.compatb[by]; }
        uint32_t compat6 = 0;
        {
            int pi = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i + 1; j < 4; ++j, ++pi) compat6 |= ((cs[i] >> sy[j]) & 1u) << pi;
        }
        uint32_t h = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) h |= ((compat6 >> ((pl >> (7 * e + 4)) & 7u)) & 1u) << e;
        hits &= h;
    }
    if (dup || !on) hits = 0u;
    const uint32_t nh = (uint32_t)__popc(hits);
    if (qu.direct && qu.two()) {
        // two sub-regions: a lane's records may go either way -- slot by slot through put_rec (two ballots and ranks each)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool he = (hits >> e) & 1u;
            if (e >= 2 && !__ballot(he)) continue;                            // wave-uniform
            const uint32_t rp = (pl >> (7 * e)) & 3u, gp = (pl >> (7 * e + 2)) & 3u;
            const uint32_t gd = L.da[p + gp] - a.n_reads;
            put_rec(qu, a, checked(qu, he, genome_ok(gd, a.n_refs)), L.da[p + rp], gd);
        }
        return nh + nflush;
    }
    const uint32_t incl_all = wave_incl_scan(nh), total_all = rl32(incl_all, 63);
    // a batch adds at most 4 entries per lane = 256; where the queue is shorter than that (the 16-wave EBWT=1 kernel) a batch
    // that cannot fit even an emptied queue goes in two halves, slots 0..1 then 2..3 of the pair lists (at most 128 each)
    const uint32_t halves = total_all + 2u * 15u > qu.cap ? 2u : 1u;          // wave-uniform (a binned drain leaves up to 2 x 15 records behind in its line buffers, not in the queue)
#pragma unroll 1
    for (uint32_t half = 0; half < halves; ++half) {
        const uint32_t hp = halves == 1u ? hits : (half ? hits & 12u : hits & 3u);
        const uint32_t nhp = (uint32_t)__popc(hp);
        const uint32_t incl = halves == 1u ? incl_all : wave_incl_scan(nhp), total = halves == 1u ? total_all : rl32(incl, 63);
        // direct mode: ends after one call -- drain() is a room flush, which leaves qu.n <= 15 whatever the window's top left waiting (up to 63),
        // and total <= 256 with total + 30 <= cap (one half) or total <= 128 (two halves; 15 + 128 <= QCAP_SCAN_SHORT): static_asserts at flush_direct
        while (qu.n + total > qu.cap) drain(qu, a);
        const uint32_t slot0 = qu.n + incl - nhp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool he = (hp >> e) & 1u;
            if (e >= 2 && !__ballot(he)) continue;                            // wave-uniform: most rounds have no cluster with 3 or 4 pairs
            if (he) {
                const uint32_t rp = (pl >> (7 * e)) & 3u, gp = (pl >> (7 * e + 2)) & 3u;
                const uint32_t slot = (EBWT || halves != 1u) ? slot0 + (uint32_t)__popc(hp & ((1u << e) - 1u)) : slot0 + (uint32_t)e;
                // (the slot is given out already: a genome index beyond the table leaves a stand-in there -- cell 0 / an entry that adds 0)
                const uint32_t gd = L.da[p + gp] - a.n_reads;
                const bool ok = checked(qu, true, genome_ok(gd, a.n_refs));
                if (qu.direct) {                                              // (one sub-region: the finished record)
                    qu.qr[slot] = rec_or_stand_in(ok, L.da[p + rp], gd, a.n_refs);
                } else {
                qu.qr[slot] = L.da[p + rp];
                qu.qg[slot] = entry_or_stand_in(ok, gd, T_SHIFT);
                }
            }
        }
        qu.n += total;
    }
    return nh + nflush;
}

// Clusters of 5..SMALL_MAX symbols by ROWS in fixed lane groups: G lanes per cluster (G = 8 for 5..8 symbols, 16 for
// 9..16), lane i of a group = position i of its cluster -- no prefix sums, no flags in LDS, and all rows of a cluster
// sit in one pass.  A row compares its document with those of the positions after it (equal: the whole cluster goes to
// the repeat store -- the group learns it from one ballot) and, if it is of the cluster's MORE COMMON kind, emits its
// pairs with the elements of the rarer kind, before and after it: the emission loop runs min(reads, genomes) times
// (usually once) instead of once per partner of a lone read.  `list`: entries position | (len-1) << 12.
template <int EBWT, int G, typename LDS>
__device__ __forceinline__ uint32_t score_rows3(LDS &L, const WgTables &T, UpdQueue &qu, uint32_t &n_dup, const ScanArgs &a,
                                                const uint16_t *list, uint32_t n)
{
    constexpr uint32_t LG = G == 8 ? 3u : 4u, PER = 64u / (uint32_t)G;
    static_assert(G == 8 || G == 16, "groups of 8 or 16 lanes");
    const uint32_t lane = lane_id(), g = lane >> LG, i = lane & ((uint32_t)G - 1u);
    uint32_t nupd = 0;
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < n; c0 += PER) {
        const bool valid = c0 + g < n;
        const uint32_t it = valid ? list[c0 + g] : 0u;                          // one address per group: a broadcast read
        const uint32_t p = it & 0xFFFu, cl = valid ? (it >> 12) + 1u : 0u;
        const bool on = i < cl;
        const uint32_t q = p + i;
        const uint32_t di = L.da[q];
        const uint32_t clm = (1u << cl) - 1u;
        const uint32_t rbc = bits_at(L.rb, p) & clm;                            // the cluster's read bits
        uint32_t dupb = 0;
#pragma unroll
        for (int k = 1; k < G; ++k) dupb |= (uint32_t)(L.da[q + (uint32_t)k] == di) << k;
        const uint32_t rem = on ? cl - 1u - i : 0u;                             // positions after i in the cluster
        const uint64_t dm = __ballot(on && (dupb & ((2u << rem) - 2u)));
        const bool gdup = (uint32_t)(dm >> (lane & ~((uint32_t)G - 1u))) & ((1u << G) - 1u);    // a row of my group met its document again
        const uint32_t ri = (rbc >> i) & 1u, nr = (uint32_t)__popc(rbc);
        const bool reads_common = 2u * nr > cl;
        // rows of the more common kind emit; partners: the elements of the other kind
        uint32_t partners = (on && !gdup && (ri != 0u) == reads_common) ? (ri ? ~rbc & clm : rbc) : 0u;
        const uint32_t ci = EBWT ? T.compatb[L.fl[q]] : 0xFFFFu;
        while (__ballot(partners != 0u)) {
            const bool act = partners != 0u;
            const uint32_t k = act ? (uint32_t)__builtin_ctz(partners) : 0u;
            partners &= partners - 1u;
            const uint32_t dj = L.da[p + k];
            bool hit = act;
            if (EBWT) hit = act && ((ci >> T.symidx[L.fl[p + k]]) & 1u);
            const uint32_t gd = (ri ? dj : di) - a.n_reads;
            hit = checked(qu, hit, genome_ok(gd, a.n_refs));
            if (qu.direct) { put_rec(qu, a, hit, ri ? di : dj, gd); nupd += (uint32_t)hit; continue; }
            const uint64_t m = __ballot(hit);
            while (qu.n + 64u > qu.cap) drain(qu, a);
            if (hit) {
                const uint32_t slot = qu.n + rank_in(m);
                qu.qr[slot] = ri ? di : dj;
                qu.qg[slot] = gd | (1u << T_SHIFT);
            }
            qu.n += (uint32_t)__popcll(m);
            nupd += (uint32_t)hit;
        }
        if (dm) nupd += dup_push<EBWT>(L, n_dup, a, T, qu, valid && gdup && i == 0u, p, cl);
    }
    return nupd;
}

// ---- window loads: lane l holds positions 64 j + l (j < PPL) of the window -- every load
// instruction reads 64 consecutive elements, and the wave ballot of a comparison on register j IS
// mask word j -- the ebwt bytes 256 k + 4 l .. + 3 (k < PPL/4), and position WIN + l of the
// read-ahead (lanes < HALO).  Elements at or beyond n_avail read as 0.
struct WinRegs { uint32_t lv[PPL], dv[PPL], bv[PPL / 4], hl, hd, hb; };
typedef uint32_t __attribute__((may_alias, aligned(1))) u32u;    // ebwt words: any byte alignment

// the three input arrays are read once: non-temporal loads keep them from displacing the score table
// (the target of the compare-and-swaps) in the caches
#ifdef LIME_PLAIN_LOADS
#define LIME_STREAM_LOAD(p) (*(p))
#else
#define LIME_STREAM_LOAD(p) __builtin_nontemporal_load(p)
#endif

template <int EBWT>
__device__ __forceinline__ void window_load(WinRegs &t, const ScanArgs &a, uint64_t lo)
{
    const uint32_t lane = lane_id();
    const ScanArgs &c = EBWT ? cold(a) : a;                // EBWT = 1 (SGPRs short): array pointers and length as scalar loads per window, not held through the loop
    const uint32_t *lp = c.lcp + lo + lane, *dp = c.da + lo + lane;
    if (lo + WIN <= c.n_avail) {                           // wave-uniform: the whole window is data
#pragma unroll
        for (int j = 0; j < (int)PPL; ++j) { t.lv[j] = LIME_STREAM_LOAD(lp + 64 * j); t.dv[j] = LIME_STREAM_LOAD(dp + 64 * j); }
#pragma unroll
        for (int k = 0; k < (int)PPL / 4; ++k)
            t.bv[k] = EBWT ? LIME_STREAM_LOAD(reinterpret_cast<const u32u *>(c.ebwt + lo + 256u * (uint32_t)k + 4u * lane)) : 0u;
    } else {
        // the last window of the data: addresses clamped to the last element (what the padding
        // positions read is never used: the masks mark them), ebwt byte by byte
        const uint64_t left = c.n_avail > lo ? c.n_avail - lo : 0ull;      // valid positions of the window (> 0)
        const uint32_t last = (uint32_t)left - 1u;
#pragma unroll
        for (int j = 0; j < (int)PPL; ++j) {
            const uint32_t p = 64u * (uint32_t)j + lane, q = p < last ? p : last;
            t.lv[j] = c.lcp[lo + q]; t.dv[j] = c.da[lo + q];
            // opaque to the optimiser: otherwise it folds these loads with the fast path's into one load
            // through a selected 64-bit address per register (32 address pairs of VGPRs, no `nt`)
            asm volatile("" : "+v"(t.lv[j]), "+v"(t.dv[j]));
        }
#pragma unroll
        for (int k = 0; k < (int)PPL / 4; ++k) {
            uint32_t w = 0;
            if (EBWT)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t p = 256u * (uint32_t)k + 4u * lane + (uint32_t)b;
                    w |= (uint32_t)c.ebwt[lo + (p < last ? p : last)] << (8 * b);
                }
            asm volatile("" : "+v"(w));
            t.bv[k] = w;
        }
    }
    const uint64_t hp = lo + WIN + lane;
    const bool hok = lane < HALO && hp < c.n_avail;
    t.hl = hok ? c.lcp[hp] : 0u;
    t.hd = hok ? c.da[hp] : 0u;
    t.hb = (EBWT && hok) ? c.ebwt[hp] : 0u;
}

// =========================================================================================
// k_scan: the streaming scan.  Every wave is an independent worker over windows of WIN positions; a workgroup (one per
// CU) takes chunks of as many consecutive windows as it has waves, which draw them from an LDS counter; no workgroup
// barrier in the loop.
// MODE 0: detect + score; 1: count clusters per window and keep the window's masks for k_emit.
// Front end: lane-strided loads; mask words from wave ballots; lane l owns the CHUNK of positions
// [16 l, 16 l + 16): its head / read bits are 16-bit masks cut out of the mask words, cluster
// acceptance inside a chunk is a carry ripple on 16 bits (32-bit arithmetic), the segment of a
// chunk's LAST head is decided with wave ballots over "chunk has a head / a read / a genome" and
// one ds_bpermute, the read-ahead being one more chunk (wave-uniform).  Every lane then writes
// (position, length) of its accepted clusters into an LDS list at the slots a wave prefix sum gives
// it; the scoring rounds read that list 64 clusters at a time.
// =========================================================================================
template <int EBWT, int BIN>                 // EBWT == 0: no symbols are staged (a kilobyte less per wave); BIN: the line buffers of the record drains
struct alignas(16) ScanLdsT {
    uint32_t da[WPOS + SMALL_MAX];
    uint8_t fl[EBWT ? WPOS + SMALL_MAX : 16];
    alignas(8) uint8_t hb[WPOS / 8 + 14];    // head / read bit of every staged position (byte k = positions 8k..8k+7)
    alignas(8) uint8_t rb[WPOS / 8 + 14];
    // accepted clusters of the window, in order: start | min(len, 63) << 10.  The scoring rounds read it 64
    // entries at a time and write the list of the clusters of 5..SMALL_MAX symbols (start | (len-1) << 12) over
    // its already consumed head: the k-th such cluster is at most the k-th cluster read.
    uint16_t listM[WIN / 2];
    uint16_t m_tstart[64];                   // the round's clusters of 9..SMALL_MAX symbols (position | (len-1) << 12)
    static constexpr uint32_t QCAP = EBWT ? QCAP_SCAN_SHORT : QCAP_SCAN;
    uint32_t q_read[QCAP], q_gen[QCAP];
    uint32_t sub_n[MAX_SUB + 1];             // binned updates: records in each of the wave's sub-regions; [MAX_SUB]: offset of the wave's producer group in the workgroup's bin histogram
    uint32_t lfill[2], lbuf[BIN ? 2 * LBUF : 2];   // records waiting for their 64-byte line (drain_lines)
    uint32_t g_doc[EBWT ? DUP_SLOTS_E : DUP_SLOTS][SMALL_MAX];
    uint8_t g_sym[EBWT ? DUP_SLOTS_E : 1][SMALL_MAX], g_len[DUP_SLOTS];
    static constexpr uint32_t NDUP = EBWT ? DUP_SLOTS_E : DUP_SLOTS;
};

struct Ctx16 {
    uint32_t h, r, g;   // 16-bit masks of this lane's chunk
    uint32_t ah;        // heads of accepted, owned clusters that close inside window + read-ahead
    uint32_t e_suf;     // window position where the segment of the chunk's last head ends (NONE32: open)
    uint64_t HW, RW, GW;  // chunk has a head / a read / a genome (wave ballots)
    uint32_t info;      // fh | lh << 5 | pre_r << 10 | pre_g << 11 | suf_r << 12 | suf_g << 13
};

// An owned run that is still open where the shard's arrays end, with more of the collection behind them
// (ClusterLCP.cpp:246-264 would read on).  Longer than LIME_MAX_CLUSTER already: if it holds a read and a genome
// it is a cluster ClusterBWT_DA refuses (:558-562) -- error now; else whether it becomes one is decided by the
// shards after this one: leave its content in the shard's edge word for the host to combine (lime_combine_edges).
// Shorter (a caller with a halo below LIME_MAX_CLUSTER): cannot be decided here -> LIME_FLAG_HALO.
__device__ __forceinline__ void open_run_at_end(const ScanArgs &a, uint64_t len_so_far, bool has_r, bool has_g)
{
    if (len_so_far <= LIME_MAX_CLUSTER) { atomicOr(&cold(a).stats->flags, LIME_FLAG_HALO); return; }
    if (has_r && has_g) { atomicOr(&cold(a).stats->flags, LIME_FLAG_MAXLEN); return; }
    atomicOr(cold(a).edge, LIME_EDGE_OPEN | (has_r ? LIME_EDGE_OPEN_R : 0u) | (has_g ? LIME_EDGE_OPEN_G : 0u));
}

// H64 / R64 / G64: the read-ahead chunk (16 bits, wave-uniform).  own_lim <= WIN.
__device__ __forceinline__ Ctx16 chunk_context(uint32_t h, uint32_t r, uint32_t g, uint32_t H64, uint32_t R64, uint32_t G64,
                                                uint32_t own_lim)
{
    const uint32_t lane = lane_id();
    Ctx16 c;
    c.h = h; c.r = r; c.g = g;
    const bool has_h = h != 0u;
    c.HW = __ballot(has_h); c.RW = __ballot(r != 0u); c.GW = __ballot(g != 0u);
    const uint32_t fh = has_h ? (uint32_t)__builtin_ctz(h) : 16u;
    const uint32_t lh = has_h ? 31u - (uint32_t)__builtin_clz(h) : 0u;
    const uint32_t lowm = (1u << fh) - 1u;                                        // headless: the whole chunk
    const uint32_t pre_r = (r & lowm) != 0u, pre_g = (g & lowm) != 0u;
    const uint32_t him = has_h ? ((0xFFFFu << lh) & 0xFFFFu) : 0u;
    const uint32_t suf_r = (r & him) != 0u, suf_g = (g & him) != 0u;
    c.info = fh | (lh << 5) | (pre_r << 10) | (pre_g << 11) | (suf_r << 12) | (suf_g << 13);
    const uint64_t gt = (lane == 63u) ? 0ull : (~0ull << (lane + 1u));
    const uint64_t above = c.HW & gt;
    const bool next_lane = above != 0ull;
    const uint32_t wn = next_lane ? (uint32_t)__builtin_ctzll(above) : 64u;
    const uint64_t between = gt & (wn >= 64u ? ~0ull : ((1ull << wn) - 1ull));   // headless chunks after this one
    const uint32_t mid_r = (c.RW & between) != 0ull, mid_g = (c.GW & between) != 0ull;
    const uint32_t nx = (uint32_t)__shfl((int)c.info, next_lane ? (int)wn : (int)lane);
    // no head in a later chunk of the window: the read-ahead chunk comes next
    const uint32_t hfh = H64 ? (uint32_t)__builtin_ctz(H64) : 16u, hlow = (1u << hfh) - 1u;
    const uint32_t n_r = next_lane ? (nx >> 10) & 1u : (uint32_t)((R64 & hlow) != 0u);
    const uint32_t n_g = next_lane ? (nx >> 11) & 1u : (uint32_t)((G64 & hlow) != 0u);
    const bool has_next = next_lane || H64 != 0u;
    c.e_suf = next_lane ? PPL * wn + (nx & 31u) : (H64 ? WIN + hfh : NONE32);
    const uint32_t acc_suf = (has_next && (suf_r | mid_r | n_r) && (suf_g | mid_g | n_g)) ? 1u : 0u;
    // "segment contains a read / a genome" gathered onto the segment's head bit by a carry ripple on 16
    // bits: in bit-reversed order a head is the TOP of its segment, and adding the seeds (Y) to the "may
    // receive from below" mask (Mr) ripples a carry through each segment up to its head
    const uint32_t Hr = __builtin_bitreverse32(h) >> 16, Mr = ~(Hr << 1) & 0xFFFFu;
    uint32_t Xr = __builtin_bitreverse32(r) >> 16, Y = (Xr << 1) & Mr;
    const uint32_t RH = (Xr | (((Mr + Y) ^ Mr) & Mr) | Y) & Hr;
    Xr = __builtin_bitreverse32(g) >> 16; Y = (Xr << 1) & Mr;
    const uint32_t GH = (Xr | (((Mr + Y) ^ Mr) & Mr) | Y) & Hr;
    uint32_t ah = __builtin_bitreverse32(RH & GH) >> 16;
    ah = (ah & ~(1u << lh)) | (acc_suf << lh);                     // last head: decided with the chunks after
    const uint32_t c0 = PPL * lane;                                // ownership: window part owned by this shard
    ah &= own_lim >= c0 + PPL ? 0xFFFFu : (own_lim <= c0 ? 0u : ((1u << (own_lim - c0)) - 1u));
    c.ah = has_h ? ah : 0u;
    return c;
}

// BIN 1 (MODE 0 only): table updates leave the kernel as records (binned update path) instead of compare-and-swaps.
// waves per SIMD the kernel is compiled for.  (The binned EBWT=0 scan was tried at four -- 128 VGPRs, 39.6 KB of LDS per
// workgroup with a 1024-bin histogram, no spills: same time as at three, 2.08 vs 2.10 ms on configs[2]; the scan is
// bound by the vector ALU's issue rate and the memory system together, not by latency a fourth wave would hide.)

template <int EBWT, int MODE, int BIN>
__global__ __launch_bounds__((ScanCfg<EBWT, BIN>::wg)) __attribute__((amdgpu_waves_per_eu((ScanCfg<EBWT, BIN>::waves), (ScanCfg<EBWT, BIN>::waves)))) void k_scan(ScanArgs a)
{
    constexpr int SCANK_WG = ScanCfg<EBWT, BIN>::wg;
    static_assert(BIN == 0 || MODE == 0, "records are made by the scoring scan only");
    static_assert(BIN >= 0 && BIN <= 2, "0: compare-and-swap; 1: records through the update queue (any number of sub-regions); 2: records written by the scorers (one or two sub-regions)");
    typedef ScanLdsT<EBWT, BIN> ScanLds;
    __shared__ ScanLds lds[SCANK_WG / 64];
    __shared__ WgTables T;
    // per wave the in-flight compare-and-swap slots (entry read, genome | t, expected word: 3 x 64 NJ words, NJ slots per
    // lane: 4, or 2 in the 8-wave workgroup); in binned mode the workgroup's histogram of update records per table bin instead
    constexpr uint32_t NJ = SCANK_WG > 256 ? 2u : 4u;
    constexpr uint32_t FS = BIN ? BIN_MAX : (SCANK_WG / 64) * 192u * NJ;
    __shared__ uint32_t fslots[FS];
    __shared__ uint32_t wg_done, wg_next, wg_exit, wg_max_len, wg_rec_max;
    __shared__ unsigned long long wg_n_clusters, wg_n_updates;
    __shared__ uint64_t wg_slot[16];
    const uint32_t lane = lane_id(), wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: LDS bases stay scalar
    ScanLds &L = lds[wave];
    constexpr bool binned = BIN != 0;
    if (binned) {
        for (uint32_t i = threadIdx.x; i < FS; i += SCANK_WG) fslots[i] = 0u;
        if (threadIdx.x == 0) wg_done = 0u;
    }
    if (threadIdx.x == 0) { wg_next = 0u; wg_exit = 0u; wg_max_len = 0u; wg_rec_max = 0u; wg_n_clusters = 0ull; wg_n_updates = 0ull; }
    if (threadIdx.x < 16) wg_slot[threadIdx.x] = 0ull;
    tables_init(T);                                        // the only workgroup barrier of the kernel
    const uint32_t n_win = a.n_tiles;
    constexpr uint32_t WPW = SCANK_WG / 64;
    UpdQueue qu; qu.qr = L.q_read; qu.qg = L.q_gen; qu.n = 0; qu.cap = ScanLds::QCAP;
    qu.async = true;
    if (!binned) { qu.nj = NJ; qu.fr = fslots + 192u * NJ * wave; qu.fg = qu.fr + 64u * NJ; qu.fe = qu.fr + 128u * NJ; }
    const uint32_t wave_gid = blockIdx.x * (SCANK_WG / 64) + wave;
    qu.binned = binned;
    qu.direct = BIN == 2;
    if (BIN == 2) {
        qu.sub_rb = cold(a).sub_rb; qu.sub_gb = cold(a).sub_gb;             // (sub_rb = ~0 for one sub-region: fused_dev_impl)
    }
    if (binned) {
        // the workgroup's waves count their records in groups of prod_waves: every group is one "producer" of k_part (more, smaller
        // producers = more partition workgroups per CU); the groups' histograms lie one after the other
        qu.out = cold(a).pool + (size_t)wave_gid * cold(a).n_sub * cold(a).cap_w; qu.hist = fslots; qu.sub_n = (lds_vu32 *)L.sub_n;
        qu.lbuf = L.lbuf; qu.lfill = (lds_vu32 *)L.lfill;
        if (lane < MAX_SUB) L.sub_n[lane] = 0u;
        if (lane < 2u) L.lfill[lane] = 0u;
        if (lane == 0u) L.sub_n[MAX_SUB] = (wave / cold(a).prod_waves) * cold(a).n_bins;   // where this wave's group counts (read back per drain: held in a register it costs the loop an SGPR)
    }
    // binned mode, end of a wave: its record count; the workgroup's last wave writes the bin histogram
    auto finish_binned = [&]() {
        const uint32_t n_sub = cold(a).n_sub, cap_w = cold(a).cap_w;
        if (lane < n_sub) {
            const uint32_t n = BIN == 2 ? (lane ? qu.base1 : qu.base0) : qu.sub_n[lane];
            cold(a).wave_cnt[(size_t)(blockIdx.x * (SCANK_WG / 64) + wave) * n_sub + lane] = n < cap_w ? n : cap_w;
            atomicMax(&wg_rec_max, n);
            if (n > cap_w) {                                 // the pass's first overflow also counts the pass as unsettled
                const uint32_t old = atomicOr(&cold(a).stats->flags, LIME_FLAG_POOL_FULL);
                if (!(old & LIME_FLAG_POOL_FULL)) atomicAdd(cold(a).sticky, 1u);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        uint32_t old = 0;
        if (lane == 0) old = atomicAdd(&wg_done, 1u);
        old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
        if (old == SCANK_WG / 64 - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const uint32_t nb = cold(a).n_bins, H = (uint32_t)(SCANK_WG / 64) / cold(a).prod_waves, np = gridDim.x * H;
            for (uint32_t i = lane; i < nb * H; i += 64u) {
                const uint32_t h = i / nb, b = i - h * nb;
                cold(a).counts[(size_t)b * np + blockIdx.x * H + h] = fslots[i];
            }
        }
    };
    // The workgroup takes chunks of its wave count of consecutive windows and its waves draw the windows of those chunks
    // one by one from an LDS counter: the waves of a CU do not run equally fast (with every wave on a fixed share,
    // configs[2], the older wave of each SIMD's pairs ended at 0.70 .. 0.78 of the kernel's time and the tail ran at a
    // fraction of the occupancy); drawn this way they end within a window of each other.  The chunks of the first
    // n_static rounds go round-robin over the workgroups; the XCDs do not run equally fast either (the odd ones ended 5 ..
    // 9 % later), so the chunks of the last rounds come from a device-wide counter, one atomic per chunk: the wave that
    // draws the first window of chunk k fetches chunk k + 1 and leaves it, tagged k + 2, in the LDS slot the others poll.
    auto take = [&]() -> uint32_t {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(&wg_next, 1u);
        i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
        const uint32_t ksw = cold(a).n_static, ks = ksw & 0xFFFFFFu, ps = ksw >> 24;   // rounds of round-robin chunks | probe shift << 24
        const uint32_t k = i / WPW, j = i % WPW;
        uint32_t chunk = k * gridDim.x + blockIdx.x;
        if (k >= ks) {
            // slot k & 15 carries the tags k + 1 - 16 (or 0), k + 1, k + 1 + 16, ... in turn.  A wave that finds a LATER tag than its own was
            // parked, between its draw and this read, while its workgroup went through 16 more chunks: its chunk's number is gone.
            // Practically out of reach (every other wave of the workgroup would have to draw 16 windows meanwhile), but a spin
            // without an exit is not: such a wave -- or one that has polled for seconds -- flags the pass as failed and stops.
            uint64_t v;
            uint32_t spins = 0;
            for (;;) {
                v = __hip_atomic_load(&wg_slot[k & 15u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const uint32_t tag = (uint32_t)(v >> 32);
                if (tag == k + 1u) break;
                if (tag > k + 1u || ++spins > (1u << 24)) {
                    if (lane == 0) atomicOr(&cold(a).stats->flags, LIME_FLAG_INTERNAL);
                    return NONE32;                     // >= n_win: the wave ends
                }
                __builtin_amdgcn_s_sleep(2);
            }
            chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
        }
        // (after chunk k is known: the workgroup's fetches follow each other, so its chunks ascend and a wave that draws a
        // window past the end can stop -- no chunk fetched later is still inside)
        if (j == 0u && k + 1u >= ks) {
            if (lane == 0) {
                const uint32_t g = atomicAdd(cold(a).dyn, 1u);
                __hip_atomic_store(&wg_slot[(k + 1u) & 15u], ((uint64_t)(k + 2u) << 32) | (uint64_t)(ks * gridDim.x + g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        return (chunk << ps) * WPW + j;                // (ps != 0: the density probe scans every 2^ps-th chunk only)
    };
    // end of a wave.  The counters of the pass are summed per workgroup in LDS and its last wave adds them to the device's:
    // the waves end together, and a few atomics per wave on the same few words took the last 0.1 .. 0.2 ms of the kernel
    // (configs[2]: 16 k atomics on one cache line).  The last wave of the last workgroup leaves the chunk counters at 0
    // for the next launch.
    auto wave_exit = [&](uint32_t tn, uint32_t tm, uint32_t tu) {
        if (lane == 0) {
            if (tn) atomicAdd(&wg_n_clusters, (unsigned long long)tn);
            if (tm) atomicMax(&wg_max_len, tm);
            if (tu) atomicAdd(&wg_n_updates, (unsigned long long)tu);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (atomicAdd(&wg_exit, 1u) == WPW - 1u) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                DevStats *st = cold(a).stats;
                const unsigned long long nc = __hip_atomic_load(&wg_n_clusters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), nu = __hip_atomic_load(&wg_n_updates, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const uint32_t ml = __hip_atomic_load(&wg_max_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), rm = __hip_atomic_load(&wg_rec_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (nc) atomicAdd(&st->n_clusters, nc);
                if (ml) atomicMax(&st->max_len, (unsigned long long)ml);
                if (MODE == 0 && nu) atomicAdd(&st->n_updates, nu);
                if (rm) atomicMax(&st->wave_records_max, rm);
                uint32_t *dyn = cold(a).dyn;
                if (atomicAdd(dyn + 1, 1u) == gridDim.x - 1u) {
                    __hip_atomic_store(dyn, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(dyn + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    };
    uint32_t win = take();
    if (win >= n_win) { if (binned) finish_binned(); wave_exit(0u, 0u, 0u); return; }
    WinRegs regs;
    window_load<EBWT>(regs, a, (uint64_t)win * WIN);
    uint32_t acc_n = 0, acc_max = 0, acc_upd = 0;          // per-lane partial counters, reduced once at the end
    uint32_t n_dup = 0;                                    // clusters waiting in the wave's dup store
    PT_DECL
#ifdef LIME_WALL_TIMING
    const uint64_t pt_wall0 = wall_clock64();
#endif
    for (;;) {
        PT_WAITVM PT(0)
#ifdef LIME_WALL_TIMING
        if (lane == 0 && win < (1u << 20)) atomicAdd(&g_winmark[win], ((wave_gid + 1u) & 0xFFFFu) | 0x10000u);
#endif
        const uint64_t lo = (uint64_t)win * WIN;
        const uint64_t n_own_ = (EBWT ? cold(a) : a).n_own;
        const uint32_t own_lim = (uint32_t)(n_own_ > lo ? (n_own_ - lo < WIN ? n_own_ - lo : (uint64_t)WIN) : 0ull);
        const uint64_t lim64 = (EBWT ? cold(a) : a).n_avail - lo;             // valid positions of the window + read-ahead: [0, lim)
        const uint32_t lim = (uint32_t)(lim64 < WPOS ? lim64 : (uint64_t)WPOS);
        // the kernel arguments of the flush behind the staging: their scalar loads go out here and are back when the ~160 vector instructions
        // of the staging are through (read inside the flush they were waited for with no window load in flight: 12 us of configs[2]'s scan,
        // profiles/r07_flush_ab.txt; the registers cost no further spill)
        FlushK fk = {};
        if (BIN == 2 && MODE == 0) fk = flush_args(a);
        // ---- stage the window in LDS and build the masks.  Loads are lane-strided (register j of lane l =
        // position 64 j + l: every load instruction reads 64 consecutive elements -- a lane reading its own 16
        // positions would touch 64 cache lines per instruction), so mask word j is the wave ballot of the
        // comparison on register j; v_writelane puts word j into lane j, and lane l then takes ITS 16 bits
        // (word l / 4, bits 16 (l % 4) ..) with one 64-bit permute per mask --------------------------------
        uint32_t hb, rb, gb, vb, H64, R64, G64, Hd64;
        {
            uint32_t hlo = 0, hhi = 0, rlo = 0, rhi = 0;
            static_assert(PPL == 16 && WIN / 64 == 16, "mask words are written lane by lane below");
#define LIME_WORD(J) { const uint64_t bh = __ballot(regs.lv[J] < a.alpha), br = __ballot(regs.dv[J] < a.n_reads); \
                       write_lane4<J>(hlo, hhi, rlo, rhi, (uint32_t)bh, (uint32_t)(bh >> 32), (uint32_t)br, (uint32_t)(br >> 32)); }
            LIME_WORD(0) LIME_WORD(1) LIME_WORD(2) LIME_WORD(3) LIME_WORD(4) LIME_WORD(5) LIME_WORD(6) LIME_WORD(7)
            LIME_WORD(8) LIME_WORD(9) LIME_WORD(10) LIME_WORD(11) LIME_WORD(12) LIME_WORD(13) LIME_WORD(14) LIME_WORD(15)
#undef LIME_WORD
            const uint32_t v16 = lim > WIN ? ((1u << (lim - WIN)) - 1u) & 0xFFFFu : 0u;       // data positions of the read-ahead
            Hd64 = (uint32_t)__ballot(lane < HALO && regs.hl < a.alpha) & v16;
            R64 = (uint32_t)__ballot(lane < HALO && regs.hd < a.n_reads) & v16;
            H64 = (Hd64 | ~v16) & 0xFFFFu; G64 = v16 & ~R64;
            hlo = write_lane<16>(hlo, H64); rlo = write_lane<16>(rlo, R64);
            uint64_t h = ((uint64_t)hhi << 32) | hlo, r = ((uint64_t)rhi << 32) | rlo;
            if (lim < WPOS) {                              // the end of the data: padding closes runs, is nobody's
                const uint32_t wl = 64u * lane;
                const uint64_t v = lim >= wl + 64u ? ~0ull : (lim <= wl ? 0ull : ((1ull << (lim - wl)) - 1ull));
                if (lane < NW) { h |= ~v; r &= v; }
            }
#pragma unroll
            for (int j = 0; j < (int)PPL; ++j) L.da[64 * j + (int)lane] = regs.dv[j];
            if (EBWT)
#pragma unroll
                for (int k = 0; k < (int)PPL / 4; ++k) reinterpret_cast<u32u *>(L.fl)[64 * k + (int)lane] = regs.bv[k];
            uint32_t lane_v = lane;                         // opaque per window: the lane masks below are compared here instead of living in SGPR pairs through the loop
            asm volatile("" : "+v"(lane_v));
            if (lane_v < HALO) { L.da[WIN + lane_v] = regs.hd; if (EBWT) L.fl[WIN + lane_v] = (uint8_t)regs.hb; }      // (lane_v: these addresses are recomputed per window, not held through the loop)
            if (lane_v <= WIN / 64) {
                *reinterpret_cast<u64a *>(&L.hb[8u * lane_v]) = h;
                *reinterpret_cast<u64a *>(&L.rb[8u * lane_v]) = r;
            }
            const uint32_t sh = 16u * (lane & 3u);
            hb = (uint32_t)(shfl64(h, (int)(lane >> 2)) >> sh) & 0xFFFFu;
            rb = (uint32_t)(shfl64(r, (int)(lane >> 2)) >> sh) & 0xFFFFu;
            const uint32_t c0_ = PPL * lane;
            vb = lim >= c0_ + PPL ? 0xFFFFu : (lim <= c0_ ? 0u : ((1u << (lim - c0_)) - 1u));
            gb = vb & ~rb;
        }
        const uint32_t c0 = PPL * lane;
        // ---- the table updates queued while the PREVIOUS window was scored leave now, before the next window's loads:
        // vmcnt counts stores and atomics with the loads, so a store issued after the loads keeps the wave waiting for
        // its acknowledgement when it wants to stage the loaded window (measured on configs[2]: 0.34 of 2.06 ms with the
        // stores issued from the scoring rounds).  Issued here they are older than the loads and long done by then.
        if (MODE == 0 && !ABL(8)) {
            if (ABL(13)) { qu.n = 0; qu.n1 = 0; } else
            if (BIN == 2) flush_direct(qu, a, FLUSH_TOP, fk); else                  // whole batches of flush_gran records; the rest waits for the next window
            { report_bad(qu, a); if (binned) drain_bin(qu, a); else drain(qu, a); }
            asm volatile("" ::: "memory");                    // the loads below stay below
        }
        // ---- the next window's loads go out now and land while this one is processed ----------
        const uint32_t n_win_ = (EBWT ? cold(a) : a).n_tiles;
        const uint32_t next = take();
        if (next < n_win_) window_load<EBWT>(regs, a, (uint64_t)next * WIN);

        PT(1)
        if (!ABL(1)) {                               // LIME_ABLATE: timing experiments, cut after a phase
        const Ctx16 c = chunk_context(hb, rb, gb, H64, R64, G64, own_lim);
        // ---- the segment of the window's last head may still be open after the read-ahead (no head there): rare.
        // The scoring scan only notes it (start, what the window holds of it) for k_resolve_open, which walks the arrays
        // from the end of the window on; the detection pass keeps a summary per window for k_resolve<1> and k_emit.
        {
            if (MODE == 0) {
                if (H64 == 0u && c.HW != 0ull) {                                // wave-uniform
                    const uint32_t lw = 63u - (uint32_t)__clzll((long long)c.HW);
                    const uint32_t li = rl32(c.info, lw), last = PPL * lw + ((li >> 5) & 31u);
                    if (last < own_lim) {                                       // owned by this shard
                        const uint64_t whigh = (lw == 63u) ? 0ull : (~0ull << (lw + 1u));
                        const uint32_t suf = (((c.RW & whigh) || ((li >> 12) & 1u)) ? 1u : 0u) | (((c.GW & whigh) || ((li >> 13) & 1u)) ? 2u : 0u);
                        if (lane == 0) {
                            const uint32_t k = atomicAdd(&cold(a).stats->n_open, 1u);  // at most one per window: the list holds n_tiles records
                            OpenRec orec; orec.start = lo + last; orec.flags = suf; orec.pad = 0u;
                            cold(a).open[k] = orec;
                        }
                    }
                }
            } else {
            TileSummary sm;
            sm.first_head = NONE32; sm.last_head = NONE32;
            uint32_t pre = (c.RW ? 1u : 0u) | (c.GW ? 2u : 0u), suf = 0u;       // no head: the whole window is "prefix"
            if (c.HW) {                                                         // wave-uniform: scalar arithmetic
                const uint32_t fw = (uint32_t)__builtin_ctzll(c.HW), lw = 63u - (uint32_t)__clzll((long long)c.HW);
                const uint32_t fi = rl32(c.info, fw), li = rl32(c.info, lw);
                sm.first_head = PPL * fw + (fi & 31u); sm.last_head = PPL * lw + ((li >> 5) & 31u);
                const uint64_t wlow = (1ull << fw) - 1ull, whigh = (lw == 63u) ? 0ull : (~0ull << (lw + 1u));
                pre = (((c.RW & wlow) || ((fi >> 10) & 1u)) ? 1u : 0u) | (((c.GW & wlow) || ((fi >> 11) & 1u)) ? 2u : 0u);
                suf = (((c.RW & whigh) || ((li >> 12) & 1u)) ? 1u : 0u) | (((c.GW & whigh) || ((li >> 13) & 1u)) ? 2u : 0u);
            }
            if (lane == 0) { sm.pre = pre; sm.suf = suf; a.summ[win] = sm; }
            }
            // a run closed by padding instead of data while more data exists beyond the shard's
            // halo: the last data head in sight is owned and nothing but padding follows it
            if (lim < WPOS && Hd64 == 0u && !cold(a).eof) {
                const uint32_t dh = hb & vb;
                const uint64_t dw = __ballot(dh != 0u);
                if (dw) {
                    const uint32_t lw2 = 63u - (uint32_t)__clzll((long long)dw);
                    const uint32_t hl2 = rl32(dh, lw2);
                    const uint32_t bp = 31u - (uint32_t)__builtin_clz(hl2), sstar = PPL * lw2 + bp;
                    if (MODE == 1) {                           // detection alone has no length limit: the host starts over with one chunk
                        if (lane == 0 && sstar < own_lim) atomicOr(&cold(a).stats->flags, LIME_FLAG_HALO);
                    } else {
                        // what the open run holds so far: its head's chunk from the head on, the chunks after it, the read-ahead
                        const uint32_t cm = lane > lw2 ? 0xFFFFu : (lane == lw2 ? (0xFFFFu << bp) & 0xFFFFu : 0u);
                        const bool hr = __ballot((rb & vb & cm) != 0u) != 0ull || R64 != 0u;
                        const bool hg = __ballot((gb & cm) != 0u) != 0ull || G64 != 0u;
                        if (lane == 0 && sstar < own_lim) open_run_at_end(a, cold(a).n_avail - (lo + sstar), hr, hg);
                    }
                }
            }
        }
        PT(2)
        if (!ABL(3)) {
        // ---- the accepted clusters of the window: every lane lists the positions of its chunk's accepted heads at
        // the slots a wave prefix sum gives it (a short loop over its <= 8 head bits: six vector instructions a turn;
        // lengths are taken from the staged head bits later, by full waves) --------------------------------------
        const uint32_t cnt = (uint32_t)__popc(c.ah);
        const uint32_t incl = wave_incl_scan(cnt);
        const uint32_t total = rl32(incl, 63);
        acc_n += cnt;
#ifdef LIME_DEBUG_CNT          // debug builds: the window's count of accepted clusters (tools/dbg_golden.py reads it back)
        if (MODE == 0 && lane == 0) a.tile_cnt[win] = total;
#endif
        if (MODE == 0) {
            // A dense window (more than 64 accepted clusters; real collections: hundreds, 98 % of them of 2 symbols) lists its 2-symbol clusters
            // apart: such a cluster is an accepted, owned head (c.ah) followed by a non-head and a head -- bits b + 1, b + 2 of the chunk's head
            // mask, the last two from the next chunk's (behind the last chunk: the read-ahead's).  The other clusters come first in the list,
            // the 2-symbol ones behind them: listM[total - total2 .. total).
            const bool defer = total > cold(a).dense_min;                       // (64; tests: 0 = every window)
            uint32_t m2c = 0, total2 = 0, k2 = 0;
            if (defer) {                                                        // wave-uniform
                uint32_t lv = lane;                                             // (opaque per window: the shuffle index is not held through the loop)
                asm volatile("" : "+v"(lv));
                const uint32_t nb = (uint32_t)__shfl((int)(c.h & 3u), (int)((lv + 1u) & 63u));
                const uint32_t h18 = c.h | ((lv == 63u ? H64 & 3u : nb) << 16);
                m2c = c.ah & ~(h18 >> 1) & (h18 >> 2);
                const uint32_t cnt2 = (uint32_t)__popc(m2c), incl2 = wave_incl_scan(cnt2);
                total2 = rl32(incl2, 63);
                k2 = (total - total2) + (incl2 - cnt2);
                acc_max = m2c && acc_max < 2u ? 2u : acc_max;
                {
                    uint32_t m = c.ah, k = (incl - cnt) - (incl2 - cnt2);
                    while (__ballot(m != 0u)) {
                        if (m) {
                            const uint32_t b = (uint32_t)__builtin_ctz(m);
                            const bool two = (m2c >> b) & 1u;
                            L.listM[two ? k2 : k] = (uint16_t)(c0 | b);
                            k2 += (uint32_t)two; k += (uint32_t)!two;
                            m &= m - 1u;
                        }
                    }
                }
            } else {
                uint32_t m = c.ah, k = incl - cnt;
                while (__ballot(m != 0u)) {
                    if (m) { L.listM[k++] = (uint16_t)(c0 | (uint32_t)__builtin_ctz(m)); m &= m - 1u; }
                }
            }
            PT(3)
            // Rounds of 64 clusters.  First the 2-symbol clusters of a dense window (listed apart: positions only, one pair each), then the others:
            // a round reads 64 positions, takes every cluster's length from the head bits (the next head after it), scores the short ones
            // (<= 4 symbols) at once and files those of 5..SMALL_MAX symbols (position | (len-1) << 12, over the already consumed head of the
            // list) for the rows routine.
            uint32_t nM = 0;
            const uint32_t n_rest = total - total2;
            if (!ABL(4) && !ABL(10))
#pragma unroll 1
            for (uint32_t base = 0; base < total2; base += 64u) {
                const uint32_t t = base + lane;
                const bool on = t < total2;
                const uint32_t p = on ? (uint32_t)L.listM[n_rest + t] & 0xFFFu : 0u;
                acc_upd += score_len2<EBWT>(L, T, qu, a, on, p);
            }
            if (!ABL(4) && !ABL(12))
#pragma unroll 1
            for (uint32_t base = 0; base < n_rest; base += 64u) {
                const uint32_t t = base + lane;
                const bool on = t < n_rest;
                const uint32_t item = on ? L.listM[t] : 0u;
                const uint32_t p = item & 0xFFFu;
                uint32_t len;
                {
                    const uint32_t w = bits_at(L.hb, p + 1u);             // head bits of p+1 .. p+32
                    len = w ? (uint32_t)__builtin_ctz(w) + 1u : 33u;
                    if (!on) len = 0u;
                    if (__ballot(len > SMALL_MAX)) {
                        if (len >= 33u) {                                 // rare: walk the head bytes to the end of the run
                            uint32_t q = p + 33u, e = WPOS;               // an accepted cluster closes before WPOS
                            while (q < WPOS) {
                                const uint32_t hbq = (uint32_t)L.hb[q >> 3] >> (q & 7u);
                                if (hbq) { e = q + (uint32_t)__builtin_ctz(hbq); break; }
                                q = (q | 7u) + 1u;
                            }
                            len = e - p;
                            if (len > MID_MAX) {                          // one workgroup per such cluster later
                                const uint32_t kk = atomicAdd(&cold(a).stats->n_big, 1u);
                                if (kk < cold(a).big_cap) { cold(a).big[kk].pStart = lo + p; cold(a).big[kk].len = len; }
                            }
                        }
                        // SMALL_MAX+1 .. MID_MAX symbols (rare): the whole wave is one lane group on the staged window, one cluster at a time
                        uint64_t mX = __ballot(len > SMALL_MAX && len <= MID_MAX);
                        while (mX) {
                            const uint32_t src = (uint32_t)__builtin_ctzll(mX);
                            mX &= mX - 1ull;
                            const uint32_t p0 = rl32(p, src), len0 = rl32(len, src);
                            const bool hvv = lane < len0;
                            acc_upd += group_score<EBWT, 64>(a, T, qu, hvv ? L.da[p0 + lane] : 0u, (EBWT && hvv) ? L.fl[p0 + lane] : 0u, len0);
                        }
                    }
                    acc_max = len > acc_max ? len : acc_max;
                }
                PT(4)
                if (ABL(10)) continue;
                const bool cM = len > 4u && len <= 8u;                     // rows in groups of 8 lanes, after the rounds
                const uint64_t mM = __ballot(cM);
                if (mM) {
                    if (cM) L.listM[nM + rank_in(mM)] = (uint16_t)(p | ((len - 1u) << 12));
                    nM += (uint32_t)__popcll(mM);
                }
                const bool cL = len > 8u && len <= SMALL_MAX;              // rare: groups of 16 lanes, at once (the list holds one round's worth)
                const uint64_t mL = __ballot(cL);
                const bool sm4 = len >= 2u && len <= 4u;
                acc_upd += score_small3<EBWT>(L, T, qu, n_dup, a, sm4, sm4 ? p : 0u, sm4 ? len : 0u);
                if (mL && !ABL(11)) {
                    if (cL) L.m_tstart[rank_in(mL)] = (uint16_t)(p | ((len - 1u) << 12));
                    acc_upd += score_rows3<EBWT, 16>(L, T, qu, n_dup, a, L.m_tstart, (uint32_t)__popcll(mL));
                }
                PT(5)
            }
            if (nM && !ABL(10) && !ABL(11) && !ABL(4)) acc_upd += score_rows3<EBWT, 8>(L, T, qu, n_dup, a, L.listM, nM);
            if (n_dup >= ScanLds::NDUP / 2u) acc_upd += dup_flush<EBWT>(L, n_dup, a, T, qu);
            PT(6)
        } else {
            // ---- count: records of the window, its masks for k_emit, the longest record -----------
            if (lane == 0) a.tile_cnt[win] = total;
            WinMasks &m = a.wmask[win];
            m.ah[lane] = (uint16_t)c.ah; m.h[lane] = (uint16_t)c.h; m.e_suf[lane] = c.e_suf;
            uint32_t mm = c.ah;
            while (mm) {
                const uint32_t b = (uint32_t)__builtin_ctz(mm);
                mm &= mm - 1u;
                const uint32_t p = c0 + b, hi = c.h >> (b + 1u);
                const uint32_t e = hi ? p + 1u + (uint32_t)__builtin_ctz(hi) : c.e_suf;
                acc_max = e - p > acc_max ? e - p : acc_max;
            }
        }
        }
        }
        if (next >= n_win_) break;
        win = next;
    }
    if (MODE == 0) {
        if (n_dup) acc_upd += dup_flush<EBWT>(L, n_dup, a, T, qu);
        if (BIN == 2) flush_direct(qu, a, FLUSH_FINAL);                        // everything that waits, the partial lines too
        else {
        report_bad(qu, a);
        do drain(qu, a); while (qu.n != 0u || __ballot(qu.f_pend != 0u));      // until every update has landed
        if (binned) drain_bin(qu, a, true);                                    // the records still waiting for their line
        }
        if (binned) finish_binned();
    }
#ifdef LIME_PHASE_TIMING
    PT(7)
    if (MODE == 0 && lane == 0 && wave == 0 && blockIdx.x % 181u == 0u)
        printf("blk %u: wait %llu stage %llu ctx %llu list %llu book %llu small %llu medium %llu tail %llu\n", blockIdx.x,
               (unsigned long long)pt_acc[0], (unsigned long long)pt_acc[1], (unsigned long long)pt_acc[2], (unsigned long long)pt_acc[3],
               (unsigned long long)pt_acc[4], (unsigned long long)pt_acc[5], (unsigned long long)pt_acc[6], (unsigned long long)pt_acc[7]);
#endif
    wave_exit(wave_sum(acc_n), wave_max(acc_max), wave_sum(acc_upd));
#ifdef LIME_WALL_TIMING      // debug build: when each wave started and ended (tools/pt_wall.sh)
    if (MODE == 0 && lane == 0 && wave_gid < 8192u) { g_wall[2u * wave_gid] = pt_wall0; g_wall[2u * wave_gid + 1u] = wall_clock64(); }
#endif
}

// =========================================================================================
// k_emit: the (pStart, len) records of every window, in ascending pStart, from the masks the
// count pass kept (WinMasks) and the windows' record offsets.  A wave per window; lane l walks the
// accepted heads among positions [16 l, 16 l + 16).  The record of a run that crosses the window's
// read-ahead (k_resolve) goes last: its head is the window's last.
// =========================================================================================
__global__ __launch_bounds__(256) void k_emit(ScanArgs a)
{
    const uint32_t lane = lane_id();
    const uint32_t win = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (win >= a.n_tiles) return;
    const uint64_t lo = (uint64_t)win * WIN;
    const WinMasks &m = a.wmask[win];
    const uint32_t hh = m.h[lane], e_suf = m.e_suf[lane];
    uint32_t ahb = m.ah[lane];
    const uint32_t my_n = (uint32_t)__popc(ahb);
    const uint32_t x = wave_incl_scan(my_n);
    uint64_t at = a.tile_off[win] + x - my_n;
    while (ahb) {
        const uint32_t b = (uint32_t)__builtin_ctz(ahb);
        ahb &= ahb - 1u;
        const uint32_t p = PPL * lane + b, hi = hh >> (b + 1u);
        const uint32_t e = hi ? p + 1u + (uint32_t)__builtin_ctz(hi) : e_suf;
        lime_cluster_t rec; rec.pStart = a.pos_base + lo + p; rec.len = e - p;
        a.out[at++] = rec;
    }
    if (lane == 63u) {
        const CrossRec cr = a.cross[win];
        if (cr.len) {
            lime_cluster_t rec; rec.pStart = a.pos_base + cr.start; rec.len = cr.len;
            a.out[at] = rec;                              // lane 63: `at` is past all records of the window
        }
    }
}

// =========================================================================================
// k_resolve: closes the segment that is still open after a window's read-ahead, from the
// summaries of the windows after it (the reference's straddle loop, ClusterLCP.cpp:246-264,
// and EOF closure :244-245).  One thread per window.  Such a cluster is longer than the
// read-ahead, hence longer than SMALL_MAX.  MODE 0: push to the big list; 1: record for emit.
// =========================================================================================
template <int MODE>
__global__ __launch_bounds__(256) void k_resolve(ScanArgs a)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.n_tiles) return;
    if (MODE == 1) { CrossRec z; z.start = 0; z.len = 0; a.cross[t] = z; }
    if (MODE == 0 && t == 0u) {
        // what lies before the shard's first head belongs to a run of an earlier shard: its content for the
        // host's combination of the shards' edge words
        uint32_t lead = 0;
        for (uint32_t u = 0; u < a.n_tiles; ++u) {
            const TileSummary o = a.summ[u];
            lead |= ((o.pre & 1u) ? LIME_EDGE_LEAD_R : 0u) | ((o.pre & 2u) ? LIME_EDGE_LEAD_G : 0u);
            if (o.first_head != NONE32) { if ((uint64_t)u * WIN + o.first_head < a.n_avail) lead |= LIME_EDGE_LEAD_HEAD; break; }
        }
        atomicOr(a.edge, lead);
    }
    const TileSummary me = a.summ[t];
    if (me.last_head == NONE32) return;
    const uint64_t s = (uint64_t)t * WIN + me.last_head;
    if (s >= a.n_own) return;                                   // owned by the next shard / padding
    uint32_t fl = me.suf;
    uint64_t e = a.n_avail;
    bool closed_by_data = false;
    for (uint32_t u = t + 1u; u < a.n_tiles; ++u) {
        const TileSummary o = a.summ[u];
        fl |= o.pre;
        if (o.first_head != NONE32) { e = (uint64_t)u * WIN + o.first_head; closed_by_data = true; break; }
    }
    if (e >= a.n_avail) { e = a.n_avail; closed_by_data = false; }
    if (!closed_by_data && !a.eof) {                            // still open where the shard's arrays end
        if (MODE == 1) { if (e >= ((uint64_t)t + 1u) * WIN + HALO) atomicOr(&a.stats->flags, LIME_FLAG_HALO); }   // (inside the read-ahead: k_scan saw it)
        else open_run_at_end(a, e - s, (fl & 1u) != 0u, (fl & 2u) != 0u);
        return;
    }
    if (e < ((uint64_t)t + 1u) * WIN + HALO) return;            // seen (and handled) inside the window's read-ahead
    const uint64_t len = e - s;
    if (fl != 3u || len < 2u) return;
    atomicAdd(&a.stats->n_clusters, 1ull);
    atomicMax(&a.stats->max_len, (unsigned long long)len);
    atomicAdd(&a.stats->n_cross, 1u);
    if (MODE == 1) {
        CrossRec c; c.start = s; c.len = len; a.cross[t] = c;
        a.tile_cnt[t] += 1u;
    } else {
        if (len > LIME_MAX_CLUSTER) { atomicOr(&a.stats->flags, LIME_FLAG_MAXLEN); return; }
        const uint32_t k = atomicAdd(&a.stats->n_big, 1u);
        if (k < a.big_cap) { a.big[k].pStart = s; a.big[k].len = len; }
    }
}

// =========================================================================================
// k_resolve_open (scoring scan): a wave per noted segment -- the last head of a window whose run has no head in the
// window's read-ahead.  The wave walks lcp / da from the end of that window to the run's end (the reference's straddle
// loop, ClusterLCP.cpp:246-264; EOF closure :244-245) and decides like k_resolve.  Wave 0 first leaves in the shard's
// edge word what lies before the shard's first head (it belongs to a run of an earlier shard).
// =========================================================================================
__device__ __forceinline__ void resolve_open_body(const ScanArgs &a, uint32_t block, uint32_t n_blocks)
{
    const uint32_t lane = lane_id();
    const uint32_t wave = block * 4u + (threadIdx.x >> 6), n_waves = n_blocks * 4u;
    // positions [from, n_avail): where the first head is (n_avail: none) and what the positions before it hold
    auto walk = [&](uint64_t from, uint32_t &fl) -> uint64_t {
        for (uint64_t i = from; i < a.n_avail; i += 64u) {
            const uint64_t p = i + lane;
            const bool ok = p < a.n_avail;
            const bool head = ok && a.lcp[p] < a.alpha;
            const bool isr = ok && a.da[p] < a.n_reads;
            const uint64_t mh = __ballot(head);
            const uint64_t below = mh ? ((1ull << (uint32_t)__builtin_ctzll(mh)) - 1ull) : ~0ull;
            if (__ballot(ok && isr) & below) fl |= 1u;
            if (__ballot(ok && !isr) & below) fl |= 2u;
            if (mh) return i + (uint32_t)__builtin_ctzll(mh);
        }
        return a.n_avail;
    };
    if (wave == 0) {
        uint32_t fl = 0;
        const uint64_t h0 = walk(0, fl);
        if (lane == 0) atomicOr(a.edge, ((fl & 1u) ? LIME_EDGE_LEAD_R : 0u) | ((fl & 2u) ? LIME_EDGE_LEAD_G : 0u) | (h0 < a.n_avail ? LIME_EDGE_LEAD_HEAD : 0u));
    }
    const uint32_t n_open = a.stats->n_open < a.n_tiles ? a.stats->n_open : a.n_tiles;
    for (uint32_t k = wave; k < n_open; k += n_waves) {
        const uint64_t s = a.open[k].start;
        uint32_t fl = a.open[k].flags;
        const uint64_t e = walk((s / WIN + 1u) * WIN, fl);
        if (lane != 0) continue;
        if (e >= a.n_avail && !a.eof) { open_run_at_end(a, e - s, (fl & 1u) != 0u, (fl & 2u) != 0u); continue; }   // still open where the shard's arrays end
        const uint64_t len = e - s;
        if (fl != 3u || len < 2u) continue;
        atomicAdd(&a.stats->n_clusters, 1ull);
        atomicMax(&a.stats->max_len, (unsigned long long)len);
        atomicAdd(&a.stats->n_cross, 1u);
        if (len > LIME_MAX_CLUSTER) { atomicOr(&a.stats->flags, LIME_FLAG_MAXLEN); continue; }
        const uint32_t kb = atomicAdd(&a.stats->n_big, 1u);
        if (kb < a.big_cap) { a.big[kb].pStart = s; a.big[kb].len = len; }
    }
}
__global__ __launch_bounds__(256) void k_resolve_open(ScanArgs a) { resolve_open_body(a, blockIdx.x, gridDim.x); }

// =========================================================================================
// k_scan_tiles: exclusive prefix sum of the per-tile record counts (one workgroup).
// =========================================================================================
__global__ __launch_bounds__(1024) void k_scan_tiles(const uint32_t *cnt, uint64_t *off,
                                                     uint32_t n, unsigned long long *total)
{
    constexpr uint32_t PER = 16;                       // consecutive counters per thread and round
    __shared__ uint64_t wsum[16];
    __shared__ uint64_t carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024u * PER) {
        const uint32_t i0 = base + tid * PER;
        uint32_t v[PER];
        uint64_t mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) { v[k] = (i0 + k < n) ? cnt[i0 + k] : 0u; mine += v[k]; }
        uint64_t x = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { uint64_t y = __shfl_up(x, d); if ((int)lane >= d) x += y; }
        if (lane == 63u) wsum[wave] = x;
        __syncthreads();
        uint64_t wpre = 0;
        for (uint32_t k = 0; k < wave; ++k) wpre += wsum[k];
        const uint64_t c = carry;
        uint64_t run = c + wpre + x - mine;
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) { if (i0 + k < n) off[i0 + k] = run; run += v[k]; }
        __syncthreads();
        if (tid == 1023u) carry = run;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// =========================================================================================
// Binned table updates, after the scan (upd_mode 1).  The scan left, per producer workgroup p and table
// bin b, the number of update records p's waves wrote to the pool (counts[b][p]) and the records
// themselves in per-wave regions.  Reference site of the updates: ClusterBWT_DA.cpp:178-184, 243-248.
//
// k_bin_rowscan: one wave per bin: counts[b][.] becomes its exclusive prefix over the producers (where p's
// records of bin b start inside the bin) and totals[b] the bin's size; k_scan_tiles turns the totals into
// bin bases.
// =========================================================================================
__global__ __launch_bounds__(256) void k_bin_rowscan(uint32_t *counts, uint32_t *totals, uint32_t n_bins, uint32_t n_prod)
{
    const uint32_t lane = lane_id();
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= n_bins) return;
    uint32_t *row = counts + (size_t)b * n_prod;
    uint32_t run = 0;
    for (uint32_t p0 = 0; p0 < n_prod; p0 += 64u) {
        const uint32_t p = p0 + lane;
        const uint32_t v = p < n_prod ? row[p] : 0u;
        const uint32_t incl = wave_incl_scan(v);
        if (p < n_prod) row[p] = run + incl - v;
        run += rl32(incl, 63);
    }
    if (lane == 0) totals[b] = run;
}

// The binned pass's two small launches behind the scan (round 5; they were four: each is 5 us of a pass whose partition takes 19 .. 160 us on the
// 10^8-symbol workloads): k_rowscan_resolve = k_bin_rowscan in its first blocks + k_resolve_open in 64 more; k_bin_bases = the bins' bases (what
// k_scan_tiles did with the totals) and, for the second level by tiles, the tiles before each bin (k_tile_bases) by one workgroup.
constexpr uint32_t RESOLVE_BLOCKS = 64;
__global__ __launch_bounds__(256) void k_rowscan_resolve(ScanArgs a, uint32_t *counts, uint32_t *totals, uint32_t n_bins, uint32_t n_prod)
{
    const uint32_t rb = (n_bins + 3u) / 4u;
    if (blockIdx.x >= rb) { resolve_open_body(a, blockIdx.x - rb, RESOLVE_BLOCKS); return; }
    const uint32_t lane = lane_id();
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= n_bins) return;
    uint32_t *row = counts + (size_t)b * n_prod;
    uint32_t run = 0;
    for (uint32_t p0 = 0; p0 < n_prod; p0 += 64u) {
        const uint32_t p = p0 + lane;
        const uint32_t v = p < n_prod ? row[p] : 0u;
        const uint32_t incl = wave_incl_scan(v);
        if (p < n_prod) row[p] = run + incl - v;
        run += rl32(incl, 63);
    }
    if (lane == 0) totals[b] = run;
}
__global__ __launch_bounds__(1024) void k_bin_bases(const uint32_t *totals, uint64_t *binbase, uint32_t *tbase, uint32_t n_bins, uint32_t tile)
{
    constexpr uint32_t PER = (BIN_MAX + 1023u) / 1024u;
    __shared__ uint64_t wsum[16];
    __shared__ uint32_t tsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, i0 = tid * PER;
    uint32_t v[PER], t[PER];
    uint64_t mine = 0; uint32_t minet = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) { v[k] = i0 + k < n_bins ? totals[i0 + k] : 0u; t[k] = (v[k] + tile - 1u) / tile; mine += v[k]; minet += t[k]; }
    uint64_t x = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint64_t y = __shfl_up(x, d); if ((int)lane >= d) x += y; }
    const uint32_t xt = wave_incl_scan(minet);
    if (lane == 63u) { wsum[wave] = x; tsum[wave] = xt; }
    __syncthreads();
    uint64_t run = x - mine; uint32_t runt = xt - minet;
    for (uint32_t k = 0; k < wave; ++k) { run += wsum[k]; runt += tsum[k]; }
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        if (i0 + k < n_bins) { binbase[i0 + k] = run; if (tbase) tbase[i0 + k] = runt; }
        run += v[k]; runt += t[k];
        if (i0 + k == n_bins - 1u) { binbase[n_bins] = run; if (tbase) tbase[n_bins] = runt; }
    }
}

// =========================================================================================
// k_score_list: scores clusters given as (pStart,len) records.  Each wave gathers 64 clusters
// (each <= SMALL_MAX long) side by side into its LDS, files them under their length class and
// runs the same scoring routines as the scan; longer clusters are pushed to the big list.
// =========================================================================================
// BIN (round 4; device-resident arrays, the table to be built from scratch): the updates leave as 4-byte records through the
// same drains, line buffers and per-bin counts as the scan's (a workgroup = one producer of k_part), instead of
// compare-and-swaps at the memory-side atomic rate -- the two-program flow on text-like density: 4.3 ms per 1e8 symbols.
template <int EBWT, int BIN>
__global__ __launch_bounds__(SCAN_WG) void k_score_list(ScanArgs a, const lime_cluster_t *list, uint64_t n_list)
{
    __shared__ WaveLds<64 * SMALL_MAX> lds[SCAN_WG / 64];
    __shared__ uint32_t c_off[SCAN_WG / 64][65];
    __shared__ uint32_t hist[BIN ? BIN_MAX : 1], bq_sub_n[SCAN_WG / 64][MAX_SUB + 1], bq_lfill[SCAN_WG / 64][2], bq_lbuf[SCAN_WG / 64][BIN ? 2 * LBUF : 2], wg_done_s;
    const uint32_t lane = lane_id(), wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: LDS bases stay scalar
    WaveLds<64 * SMALL_MAX> &L = lds[wave];
    uint32_t *off = c_off[wave];
    const uint64_t n_batches = (n_list + 63u) / 64u, stride = (uint64_t)gridDim.x * (SCAN_WG / 64);
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t acc_upd = 0;
    UpdQueue qu; qu.qr = L.q_read; qu.qg = L.q_gen; qu.n = 0; qu.cap = QCAP;
    if (BIN) {
        for (uint32_t i = threadIdx.x; i < BIN_MAX; i += SCAN_WG) hist[i] = 0u;
        if (threadIdx.x == 0) wg_done_s = 0u;
        const uint32_t wave_gid = blockIdx.x * (SCAN_WG / 64) + wave;
        qu.async = true; qu.binned = true;
        qu.out = cold(a).pool + (size_t)wave_gid * cold(a).n_sub * cold(a).cap_w; qu.hist = hist;
        qu.sub_n = (lds_vu32 *)bq_sub_n[wave]; qu.lbuf = bq_lbuf[wave]; qu.lfill = (lds_vu32 *)bq_lfill[wave];
        if (lane <= MAX_SUB) bq_sub_n[wave][lane] = 0u;               // ([MAX_SUB]: the producer group's offset in the histogram: one group)
        if (lane < 2u) bq_lfill[wave][lane] = 0u;
        __syncthreads();
    }
    for (uint64_t b = (uint64_t)blockIdx.x * (SCAN_WG / 64) + wave; b < n_batches; b += stride) {
        const uint64_t c = b * 64u + lane;
        uint64_t ps = 0, len = 0;
        if (c < n_list) { ps = list[c].pStart - a.pos_base; len = list[c].len; }      // pos_base: where the arrays handed over start in the collection
        const bool bad = (len > LIME_MAX_CLUSTER) || (ps > a.n_avail) || (len > a.n_avail - ps);
        if (bad) { atomicOr(&a.stats->flags, len > LIME_MAX_CLUSTER ? LIME_FLAG_MAXLEN : LIME_FLAG_BADCLUSTER); len = 0; }
        if (len > SMALL_MAX) {
            const uint32_t k = atomicAdd(&a.stats->n_big, 1u);
            if (k < a.big_cap) { a.big[k].pStart = ps; a.big[k].len = len; }
            len = 0;
        }
        if (len < 2u) len = 0;                     // a 0/1-symbol cluster cannot hold a read and a genome
        const uint32_t len32 = (uint32_t)len;
        uint32_t incl = len32;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(incl, d); if ((int)lane >= d) incl += y; }
        const uint32_t my_off = incl - len32, total = rl32(incl, 63);
        off[lane] = my_off;
        if (lane == 63u) off[64] = total;
        for (uint32_t i0 = 0; i0 < total; i0 += 64u) {
            const uint32_t i = i0 + lane < total ? i0 + lane : total - 1u;
            uint32_t lo = 0, hi = 63u;                // last cluster with off <= i
            while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (off[mid] <= i) lo = mid; else hi = mid - 1u; }
            const uint64_t g = shfl64(ps, (int)lo) + (i - off[lo]);
            const uint32_t d = a.da[g];
            uint32_t f = EBWT ? sym_index(a.ebwt[g]) : 0u;
            f |= (d < a.n_reads) ? F_READ : F_GEN;
            L.da[i] = d; L.fl[i] = (uint8_t)f;
            const uint64_t rm = __ballot(d < a.n_reads && i0 + lane < total);
            if (lane == 0) *reinterpret_cast<u64a *>(&L.rb[i0 >> 3]) = rm;
        }
        const bool cA = len32 >= 2u;
        const uint16_t item = (uint16_t)(my_off | ((len32 - 1u) << 12));
        const uint64_t mA = __ballot(cA);
        if (cA) L.listA[(uint32_t)__popcll(mA & lt)] = item;
        acc_upd += score_lists<EBWT>(L, qu, a, (uint32_t)__popcll(mA));
    }
    if (BIN) {                                                        // the records still waiting for their line; this wave's counts; the workgroup's histogram
        const uint32_t n_sub = cold(a).n_sub, cap_w = cold(a).cap_w;
        drain_bin(qu, a, true);
        if (lane < n_sub) {
            const uint32_t n = qu.sub_n[lane];
            cold(a).wave_cnt[(size_t)(blockIdx.x * (SCAN_WG / 64) + wave) * n_sub + lane] = n < cap_w ? n : cap_w;
            atomicMax(&cold(a).stats->wave_records_max, n);
            if (n > cap_w) atomicOr(&cold(a).stats->flags, LIME_FLAG_POOL_FULL);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        uint32_t old = 0;
        if (lane == 0) old = atomicAdd(&wg_done_s, 1u);
        old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
        if (old == SCAN_WG / 64 - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            for (uint32_t bb = lane; bb < cold(a).n_bins; bb += 64u) cold(a).counts[(size_t)bb * gridDim.x + blockIdx.x] = hist[bb];
        }
    }
    const uint32_t tu = wave_sum(acc_upd);
    if (lane == 0 && tu) atomicAdd(&a.stats->n_updates, (unsigned long long)tu);
}

// =========================================================================================
// k_score_big: one workgroup per long cluster (SMALL_MAX < len <= 65536).  Documents are
// counted in a per-workgroup open-addressing table in global scratch (it stays in L2):
// 16 x u32 counters per document, then every (read, genome) pair is scored by one lane.
// Read counts are reduced mod 256 and genome counts saturated at 255 exactly as the
// reference's unsigned chars do (ClusterBWT_DA.cpp:96-97, :123, :206, :222-223).
// =========================================================================================
__device__ __forceinline__ uint32_t ht_hash(uint32_t doc) { return (doc * 2654435761u) >> (32u - HT_BITS); }

template <int EBWT>
__global__ __launch_bounds__(WGSZ) void k_score_big(ScanArgs a, uint32_t *scratch)
{
    __shared__ uint32_t s_nr, s_ng, s_upd;
    const uint32_t tid = threadIdx.x;
    uint32_t *keys = scratch + (size_t)blockIdx.x * BIG_SCRATCH_WORDS;
    uint32_t *cnt = keys + HT_SIZE;
    uint32_t *rlist = cnt + (size_t)HT_SIZE * 16u;
    uint32_t *glist = rlist + LIME_MAX_CLUSTER;
    const uint32_t n_big = a.stats->n_big < a.big_cap ? a.stats->n_big : a.big_cap;
    for (uint32_t c = blockIdx.x; c < n_big; c += gridDim.x) {
        const uint64_t ps = a.big[c].pStart;
        const uint32_t len = (uint32_t)a.big[c].len;
        if (tid == 0) { s_nr = 0; s_ng = 0; s_upd = 0; }
        __syncthreads();
        // ---- count -------------------------------------------------------------------
        for (uint32_t p = tid; p < len; p += WGSZ) {
            const uint32_t doc = a.da[ps + p];
            const uint32_t sym = EBWT ? sym_index(a.ebwt[ps + p]) : 0u;
            uint32_t h = ht_hash(doc);
            for (;;) {
                uint32_t k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (k == HT_EMPTY) {
                    k = atomicCAS(&keys[h], HT_EMPTY, doc);
                    if (k == HT_EMPTY) {
                        if (doc < a.n_reads) rlist[atomicAdd(&s_nr, 1u)] = h;
                        else glist[atomicAdd(&s_ng, 1u)] = h;
                        break;
                    }
                }
                if (k == doc) break;
                h = (h + 1u) & (HT_SIZE - 1u);
            }
            atomicAdd(&cnt[(size_t)h * 16u + sym], 1u);
        }
        __threadfence();
        __syncthreads();
        // ---- pairs: a wave per read, lanes over genomes ---------------------------------
        const uint32_t nr = s_nr, ng = s_ng;
        const uint32_t wave = tid >> 6, lane = tid & 63u;
        uint32_t nupd = 0;
        for (uint32_t ri = wave; ri < nr; ri += WGSZ / 64) {
            const uint32_t hr = rlist[ri];
            const uint32_t rdoc = keys[hr];
            uint32_t cr[4] = {0u, 0u, 0u, 0u};
            uint32_t rcount = cnt[(size_t)hr * 16u] & 255u;
            if (EBWT) {
#pragma unroll
                for (int i = 0; i < 16; ++i) cr[i >> 2] |= (cnt[(size_t)hr * 16u + i] & 255u) << ((i & 3) * 8);
            }
            const uint64_t row = (uint64_t)rdoc * a.n_refs;
            for (uint32_t gi = lane; gi < ng; gi += 64u) {
                const uint32_t hg = glist[gi];
                const uint32_t gdoc = keys[hg];
                uint32_t t;
                if (EBWT) {
                    uint32_t cg[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        uint32_t v = cnt[(size_t)hg * 16u + i];
                        cg[i >> 2] |= (v > 255u ? 255u : v) << ((i & 3) * 8);
                    }
                    t = pair_score(cr, cg);
                } else {
                    uint32_t v = cnt[(size_t)hg * 16u];
                    v = v > 255u ? 255u : v;
                    t = rcount < v ? rcount : v;
                }
                if (t) {
                    const uint32_t g = gdoc - a.n_reads;
                    if (!genome_ok(g, a.n_refs)) atomicOr(&a.stats->flags, LIME_FLAG_DOCID);
                    else if (a.sim) { sim_add(a.sim, row + g, t); ++nupd; }
                    else {                                     // records for the owner of the cell (owner-partitioned exchange)
                        const uint32_t k = atomicAdd(a.bigrec_n, 1u);
                        if (k < a.bigrec_cap) a.bigrec[k] = (row + g) | ((uint64_t)t << CELL_BITS);
                        else atomicOr(&a.stats->flags, LIME_FLAG_OVERFLOW);
                        ++nupd;
                    }
                }
            }
        }
        if (nupd) atomicAdd(&s_upd, nupd);
        __syncthreads();
        // ---- restore the table to empty ---------------------------------------------------
        for (uint32_t i = tid; i < nr + ng; i += WGSZ) {
            const uint32_t h = i < nr ? rlist[i] : glist[i - nr];
#pragma unroll
            for (int k = 0; k < 16; ++k) cnt[(size_t)h * 16u + k] = 0u;
            keys[h] = HT_EMPTY;
        }
        __threadfence();
        __syncthreads();
        if (tid == 0 && s_upd) atomicAdd(&a.stats->n_updates, (unsigned long long)s_upd);
    }
}

// =========================================================================================
// k_choose: per read row maximum and non-zero count (clusterChoose row scan,
// ClusterBWT_DA.cpp:385-402).  One wave per row; aligned 32-bit loads over the row's bytes.
// =========================================================================================
__global__ __launch_bounds__(WGSZ) void k_choose(const uint8_t *sim, uint32_t n_reads, uint32_t n_refs,
                                                 uint8_t *row_max, uint32_t *row_nnz)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (WGSZ / 64);
    // max and non-zero count of the four bytes of a word, SWAR (no per-byte bounds checks: the caller
    // has cleared the bytes outside the row)
    auto word = [](uint32_t v, uint32_t &mx, uint32_t &nz) {
        const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24;
        const uint32_t m01 = b0 > b1 ? b0 : b1, m23 = b2 > b3 ? b2 : b3, m = m01 > m23 ? m01 : m23;
        mx = m > mx ? m : mx;
        uint32_t t = v | (v >> 4); t |= t >> 2; t |= t >> 1;
        nz += (uint32_t)__popc(t & 0x01010101u);
    };
    for (uint64_t r = (uint64_t)blockIdx.x * (WGSZ / 64) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        const uint64_t b0 = r * n_refs, b1 = b0 + n_refs;
        const uint64_t q0 = b0 >> 4, q1 = (b1 + 15ull) >> 4;            // 16-byte groups covering the row
        uint32_t mx = 0, nz = 0;
        for (uint64_t q = q0 + lane; q < q1; q += 64u) {
            uint4 v = reinterpret_cast<const uint4 *>(sim)[q];            // the table is padded to 16 bytes
            if (q == q0 || q + 1 == q1) {                                 // first / last group: clear foreign bytes
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const uint64_t byte = q * 16ull + k;
                    if (byte < b0 || byte >= b1) w[k >> 2] &= ~(255u << (8 * (k & 3)));
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            word(v.x, mx, nz); word(v.y, mx, nz); word(v.z, mx, nz); word(v.w, mx, nz);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            uint32_t om = __shfl_xor(mx, d), on = __shfl_xor(nz, d);
            mx = om > mx ? om : mx; nz += on;
        }
        if (lane == 0) { row_max[r] = (uint8_t)mx; row_nnz[r] = nz; }
    }
}

// =========================================================================================
// k_gather_pairs: the non-zero cells of the selected table rows, compacted in ascending idRef
// (the (idRef, sim) list of clusterChoose, ClusterBWT_DA.cpp:390-402).  One wave per row; cells of
// row r go to pairs[row_off[r] .. row_off[r+1]) (an empty range skips the row).
// =========================================================================================
__global__ __launch_bounds__(WGSZ) void k_gather_pairs(const uint8_t *sim, uint32_t n_reads, uint32_t n_refs,
                                                       const uint64_t *row_off, lime_pair_t *pairs)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (WGSZ / 64);
    for (uint64_t r = (uint64_t)blockIdx.x * (WGSZ / 64) + (threadIdx.x >> 6); r < n_reads; r += waves) {
        uint64_t out = row_off[r];
        if (row_off[r + 1] == out) continue;
        const uint64_t b0 = r * n_refs, b1 = b0 + n_refs;
        const uint64_t w0 = b0 >> 2, w1 = (b1 + 3ull) >> 2;
        for (uint64_t wb = w0; wb < w1; wb += 64u) {
            const uint64_t w = wb + lane;
            uint32_t v = w < w1 ? reinterpret_cast<const uint32_t *>(sim)[w] : 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {                      // bytes outside the row do not count
                const uint64_t byte = w * 4ull + k;
                if (byte < b0 || byte >= b1) v &= ~(255u << (8 * k));
            }
            const uint32_t nz = (uint32_t)((v & 0xFFu) != 0u) + (uint32_t)((v & 0xFF00u) != 0u) +
                                (uint32_t)((v & 0xFF0000u) != 0u) + (uint32_t)((v >> 24) != 0u);
            const uint32_t incl = wave_incl_scan(nz);
            uint64_t o = out + incl - nz;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t x = (v >> (8 * k)) & 255u;
                if (x) { lime_pair_t pr; pr.id_ref = (uint32_t)(w * 4ull + k - b0); pr.sim = x; pairs[o++] = pr; }
            }
            out += rl32(incl, 63);
        }
    }
}

// =========================================================================================
// k_synth: synthetic lcp/da/ebwt, element i a pure function of (seed, i0+i).
// =========================================================================================
__global__ __launch_bounds__(WGSZ) void k_synth(uint64_t seed, uint64_t i0, uint64_t count,
                                                uint32_t n_reads, uint32_t n_refs, uint32_t alpha,
                                                uint32_t mode, uint32_t *lcp, uint32_t *da, uint8_t *ebwt)
{
    const uint64_t stride = (uint64_t)gridDim.x * WGSZ;
    for (uint64_t i = (uint64_t)blockIdx.x * WGSZ + threadIdx.x; i < count; i += stride) {
        uint32_t l, d, s;
        synth_element(seed, i0 + i, n_reads, n_refs, alpha, mode, l, d, s);
        if (lcp) lcp[i] = l;
        if (da) da[i] = d;
        if (ebwt) ebwt[i] = (uint8_t)s;
    }
}

// blockIdx.y: one of gridDim.y arrays of n words, `pitch` words apart (k_score_big's scratch tables: one launch for all of them)
__global__ void k_fill_u32(uint32_t *p, size_t n, uint32_t v, size_t pitch)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    p += (size_t)blockIdx.y * pitch;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

// ---- launch wrappers (host) ------------------------------------------------------------
// ID: one per instantiation of k_scan (they share one function type, so K alone would share the static)

// (probe_shift: only every 2^probe_shift-th chunk is scanned -- the density probe)
template <int ID, int WG, typename K> static uint32_t scan_grid_of(K kernel, uint32_t n_tiles, uint32_t max_blocks, uint32_t probe_shift = 0)
{
    constexpr int SCANK_WG = WG;
    static std::atomic<uint32_t> resident_of[MAX_DEV];
    std::atomic<uint32_t> &slot = resident_of[cur_device()];
    uint32_t resident = slot.load(std::memory_order_relaxed);
    if (!resident) { resident = resident_blocks(kernel, SCANK_WG); slot.store(resident, std::memory_order_relaxed); }
    const uint32_t chunks = (n_tiles + SCANK_WG / 64 - 1) / (SCANK_WG / 64), want = (chunks + (1u << probe_shift) - 1u) >> probe_shift, cap = max_blocks ? max_blocks : resident;
    const uint32_t grid = want < cap ? want : cap;
    return grid ? grid : 1u;
}

template <int ID, int WG, typename K> static void launch_scan_kernel(K kernel, const ScanArgs &a, uint32_t max_blocks, hipStream_t st)
{
    // persistent grid: as many workgroups as fit the device at once (per instantiation), or fewer for short inputs
    const uint32_t grid = scan_grid_of<ID, WG>(kernel, a.n_tiles, max_blocks, a.probe_shift);
    const uint32_t pct = a.static_pct > 100u ? 100u : a.static_pct;
    ScanArgs b = a;
    const uint64_t chunks = (((uint64_t)a.n_tiles + WG / 64 - 1) / (WG / 64) + (1u << a.probe_shift) - 1u) >> a.probe_shift;
    const uint64_t rounds = chunks / grid;             // whole rounds of chunks
    b.n_static = (uint32_t)(rounds * (uint64_t)pct / 100u);
    if (!b.n_static) b.n_static = 1u;                  // round 0 is always the workgroups' own chunks (grid <= number of chunks)
    if (b.n_static > 0xFFFFFFu) b.n_static = 0xFFFFFFu;
    b.n_static |= a.probe_shift << 24;                 // (the kernel's take() splits the word: one SGPR for both)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(WG), 0, st, b);
}

// lime_init: every kernel's code is loaded and the launch wrappers' per-device figures (resident workgroups, LDS attributes) are worked out
// now, not inside a context's first pass (LiME_paired.sh runs a collection once: the first pass IS the run; on configs[1] the first launches'
// lazy loading and occupancy queries were 0.2 ms of a 0.25 ms pass)
void launch_preload()
{
    static std::atomic<bool> done[MAX_DEV];
    std::atomic<bool> &d = done[cur_device()];
    if (d.load(std::memory_order_relaxed)) return;
    for (int e = 0; e < 2; ++e) for (int b = 0; b < 3; ++b) (void)scan_grid(e, 0, b, 1u << 20, 0, 0);
    (void)scan_grid(0, 1, 0, 1u << 20, 0, 0);
    preload_partition(); preload_apply();
    hipFuncAttributes fa;
#define LIME_PRELOAD(K) (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(K));
    LIME_PRELOAD(k_resolve_open) LIME_PRELOAD(k_rowscan_resolve) LIME_PRELOAD(k_bin_bases) LIME_PRELOAD(k_resolve<1>) LIME_PRELOAD(k_emit) LIME_PRELOAD(k_scan_tiles) LIME_PRELOAD(k_bin_rowscan)
    LIME_PRELOAD(k_score_big<0>) LIME_PRELOAD(k_score_big<1>)
    LIME_PRELOAD(k_choose) LIME_PRELOAD(k_gather_pairs) LIME_PRELOAD((k_score_list<0, 0>)) LIME_PRELOAD((k_score_list<1, 0>))
#undef LIME_PRELOAD
    (void)hipGetLastError();
    d.store(true, std::memory_order_relaxed);
}

uint32_t scan_grid(int ebwt, int mode, int binned, uint32_t n_tiles, uint32_t max_blocks, uint32_t probe_shift)
{
    if (mode != 0) return scan_grid_of<2, ScanCfg<0, 0>::wg>(k_scan<0, 1, 0>, n_tiles, max_blocks);
    if (binned == 2) return ebwt ? scan_grid_of<6, ScanCfg<1, 2>::wg>(k_scan<1, 0, 2>, n_tiles, max_blocks, probe_shift) : scan_grid_of<5, ScanCfg<0, 2>::wg>(k_scan<0, 0, 2>, n_tiles, max_blocks, probe_shift);
    if (binned) return ebwt ? scan_grid_of<4, ScanCfg<1, 1>::wg>(k_scan<1, 0, 1>, n_tiles, max_blocks, probe_shift) : scan_grid_of<3, ScanCfg<0, 1>::wg>(k_scan<0, 0, 1>, n_tiles, max_blocks, probe_shift);
    return ebwt ? scan_grid_of<1, ScanCfg<1, 0>::wg>(k_scan<1, 0, 0>, n_tiles, max_blocks) : scan_grid_of<0, ScanCfg<0, 0>::wg>(k_scan<0, 0, 0>, n_tiles, max_blocks);
}

void launch_rowscan_resolve(const ScanArgs &a, uint32_t *counts, uint32_t *totals, uint32_t n_bins, uint32_t n_prod, hipStream_t st)
{
    hipLaunchKernelGGL(k_rowscan_resolve, dim3((n_bins + 3u) / 4u + RESOLVE_BLOCKS), dim3(256), 0, st, a, counts, totals, n_bins, n_prod);
}
void launch_bin_bases(const uint32_t *totals, uint64_t *binbase, uint32_t *tbase, uint32_t n_bins, hipStream_t st)
{
    hipLaunchKernelGGL(k_bin_bases, dim3(1), dim3(1024), 0, st, totals, binbase, tbase, n_bins, PART_TILE);
}

void launch_bin_rowscan(uint32_t *counts, uint32_t *totals, uint32_t n_bins, uint32_t n_prod, hipStream_t st)
{
    hipLaunchKernelGGL(k_bin_rowscan, dim3((n_bins + 3u) / 4u), dim3(256), 0, st, counts, totals, n_bins, n_prod);
}

void launch_tile(int ebwt, int mode, const ScanArgs &a, uint32_t max_blocks, hipStream_t st)
{
    if (mode != 0) launch_scan_kernel<2, ScanCfg<0, 0>::wg>(k_scan<0, 1, 0>, a, max_blocks, st);
    else if (a.upd_mode && a.n_sub <= 2u && !a.no_direct) {                 // the scorers write finished records (k_scan<., 0, 2>)
        if (ebwt) launch_scan_kernel<6, ScanCfg<1, 2>::wg>(k_scan<1, 0, 2>, a, max_blocks, st);
        else      launch_scan_kernel<5, ScanCfg<0, 2>::wg>(k_scan<0, 0, 2>, a, max_blocks, st);
    } else if (a.upd_mode) {
        if (ebwt) launch_scan_kernel<4, ScanCfg<1, 1>::wg>(k_scan<1, 0, 1>, a, max_blocks, st);
        else      launch_scan_kernel<3, ScanCfg<0, 1>::wg>(k_scan<0, 0, 1>, a, max_blocks, st);
    } else {
        if (ebwt) launch_scan_kernel<1, ScanCfg<1, 0>::wg>(k_scan<1, 0, 0>, a, max_blocks, st);
        else      launch_scan_kernel<0, ScanCfg<0, 0>::wg>(k_scan<0, 0, 0>, a, max_blocks, st);
    }
}

void launch_emit(const ScanArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_emit, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, st, a);
}

void launch_resolve(int mode, const ScanArgs &a, hipStream_t st)
{
    const dim3 grid((a.n_tiles + 255) / 256), block(256);
    if (mode == 0) hipLaunchKernelGGL(k_resolve_open, dim3(64), block, 0, st, a);     // a wave per noted open segment (rare), 256 waves
    else           hipLaunchKernelGGL((k_resolve<1>), grid, block, 0, st, a);
}

void launch_scan_tiles(const uint32_t *cnt, uint64_t *off, uint32_t n, unsigned long long *total, hipStream_t st)
{
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, st, cnt, off, n, total);
}

void launch_score_list(int ebwt, const ScanArgs &a, const lime_cluster_t *list, uint64_t count, uint32_t blocks, hipStream_t st)
{
    if (a.upd_mode) {
        if (ebwt) hipLaunchKernelGGL((k_score_list<1, 1>), dim3(blocks), dim3(SCAN_WG), 0, st, a, list, count);
        else      hipLaunchKernelGGL((k_score_list<0, 1>), dim3(blocks), dim3(SCAN_WG), 0, st, a, list, count);
    } else {
        if (ebwt) hipLaunchKernelGGL((k_score_list<1, 0>), dim3(blocks), dim3(SCAN_WG), 0, st, a, list, count);
        else      hipLaunchKernelGGL((k_score_list<0, 0>), dim3(blocks), dim3(SCAN_WG), 0, st, a, list, count);
    }
}

void launch_score_big(int ebwt, const ScanArgs &a, uint32_t *scratch, hipStream_t st)
{
    if (ebwt) hipLaunchKernelGGL((k_score_big<1>), dim3(BIG_GRID), dim3(WGSZ), 0, st, a, scratch);
    else      hipLaunchKernelGGL((k_score_big<0>), dim3(BIG_GRID), dim3(WGSZ), 0, st, a, scratch);
}

void launch_choose(const uint8_t *sim, uint32_t n_reads, uint32_t n_refs, uint8_t *row_max,
                   uint32_t *row_nnz, hipStream_t st)
{
    uint64_t blocks = ((uint64_t)n_reads + (WGSZ / 64) - 1) / (WGSZ / 64);
    if (blocks > 65536) blocks = 65536;
    if (!blocks) blocks = 1;
    hipLaunchKernelGGL(k_choose, dim3((uint32_t)blocks), dim3(WGSZ), 0, st, sim, n_reads, n_refs, row_max, row_nnz);
}

void launch_gather_pairs(const uint8_t *sim, uint32_t n_reads, uint32_t n_refs, const uint64_t *row_off,
                         lime_pair_t *pairs, hipStream_t st)
{
    const uint64_t want = ((uint64_t)n_reads + WGSZ / 64 - 1) / (WGSZ / 64);
    const uint32_t blocks = (uint32_t)(want < 16384u ? (want ? want : 1u) : 16384u);
    hipLaunchKernelGGL(k_gather_pairs, dim3(blocks), dim3(WGSZ), 0, st, sim, n_reads, n_refs, row_off, pairs);
}

void launch_synth(uint64_t seed, uint64_t i0, uint64_t count, uint32_t n_reads, uint32_t n_refs,
                  uint32_t alpha, uint32_t mode, uint32_t *lcp, uint32_t *da, uint8_t *ebwt, hipStream_t st)
{
    uint64_t blocks = (count + WGSZ - 1) / WGSZ;
    if (blocks > 16384) blocks = 16384;
    if (!blocks) blocks = 1;
    hipLaunchKernelGGL(k_synth, dim3((uint32_t)blocks), dim3(WGSZ), 0, st, seed, i0, count, n_reads, n_refs,
                       alpha, mode, lcp, da, ebwt);
}

__global__ void k_add_u64(uint64_t *p, size_t n, uint64_t v)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] += v;
}
void launch_add_u64(uint64_t *p, size_t n, uint64_t v, hipStream_t st)
{
    hipLaunchKernelGGL(k_add_u64, dim3(8), dim3(256), 0, st, p, n, v);
}

void launch_fill_u32(uint32_t *p, size_t n, uint32_t v, hipStream_t st, uint32_t count, size_t pitch)
{
    hipLaunchKernelGGL(k_fill_u32, dim3(count > 1 ? 64 : 1024, count), dim3(256), 0, st, p, n, v, pitch);
}

// zero a few words (the pass's counters) and, with them, a 16-byte-aligned array (the table, where the updates add to it): ONE launch.
// hipMemsetAsync is a kernel as well, but every call of it sat 10 us behind the kernel before it and 6 us in front of the next one
// in the traces (configs[1]: two calls, 30 of the pass's 264 us).
__global__ void k_zero2(uint32_t *a, uint32_t a_words, uint4 *b, size_t b_quads)
{
    if (blockIdx.x == 0) for (uint32_t i = threadIdx.x; i < a_words; i += blockDim.x) a[i] = 0u;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < b_quads; i += stride) b[i] = make_uint4(0u, 0u, 0u, 0u);
}

void launch_zero2(void *a, size_t a_bytes, void *b, size_t b_bytes, hipStream_t st)
{
    const size_t quads = b_bytes / 16u;
    const uint32_t grid = quads ? (uint32_t)((quads + 255u) / 256u < 2048u ? (quads + 255u) / 256u : 2048u) : 1u;
    hipLaunchKernelGGL(k_zero2, dim3(grid), dim3(256), 0, st, static_cast<uint32_t *>(a), (uint32_t)(a_bytes / 4u), static_cast<uint4 *>(b), quads);
}

} // namespace lime
