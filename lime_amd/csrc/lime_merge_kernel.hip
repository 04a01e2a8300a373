// lime_merge_kernel.hip -- the project's own kernels of the merge of read suffixes into a prebuilt genome index (lime_merge_index_dev,
// lime_merge.cpp), in the convention of lime_amd/builder.py and lime_index_kernel.hip.  Both sides are sorted already, each a collection
// of its own; a read suffix ends at its terminator, so its place among the genome suffixes is a bounded string search:
//   1  k_mrg_rank            j[i] = genome suffixes below read suffix i: a lower bound over the genomes' suffix array, the matched lengths
//                            at both bounds carried along (Manber-Myers), eight symbols per compare
//   2  k_mrg_ends (+ a running maximum)   c[k] = read suffixes with j <= k
//   3  k_mrg_write_reads, k_mrg_write_genomes   read i to slot i + j[i], genome k to slot k + c[k]; the lcp with a neighbour of the
//                            same side is that side's own, the lcp across the sides is compared from the two texts
// Order of a read suffix R and a genome suffix G: the first differing symbol decides (unsigned bytes); if one ends where the other goes
// on, the one that ends is below; if both end together R is below (the reads' document ids are the lower ones).
// wave64, no cross-lane operation, no inline assembly.  No kernel reads a byte outside the two texts, doc_off and the arrays it was given:
// a word is loaded only while both suffixes have eight symbols left in front of their terminators.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_index.h"

namespace lime {

namespace {

constexpr int MRG_WG = 256;
// grids are capped and every kernel strides: at most this many workgroups per launch
constexpr uint32_t MRG_RANK_BLOCKS = 8192, MRG_ENDS_BLOCKS = 8192, MRG_WRITE_BLOCKS = 8192;

__device__ __forceinline__ uint64_t load8(const uint8_t *p)
{
    uint64_t x;
    __builtin_memcpy(&x, p, 8);
    return x;
}

struct Suffix { const uint8_t *sym; uint64_t len; };         // the symbols in front of the terminator

// the suffix at slot s of a side; sa, da and the position are clamped into the side (see MrgSide)
__device__ __forceinline__ Suffix suffix_at(const MrgSide &t, uint32_t s)
{
    uint32_t p = t.sa[s], k = t.da[s];
    if (p >= t.n) p = t.n - 1u;
    if (k >= t.n_docs) k = t.n_docs - 1u;
    const uint64_t lo = t.doc_off[k] + k, hi = t.doc_off[k + 1] + k;        // the document's first position and its terminator
    const uint64_t q = p < lo ? lo : p > hi ? hi : p;
    return Suffix{t.text + (q - k), hi - q};
}

// the symbols a and b share from h on, up to lim (<= both lengths)
__device__ __forceinline__ uint64_t match_from(const uint8_t *a, const uint8_t *b, uint64_t h, uint64_t lim)
{
    if (h > lim) h = lim;
    while (h < lim) {
        if (h + 8u <= lim) {                                                // eight symbols at a time (both stay in front of their terminators)
            const uint64_t x = load8(a + h) ^ load8(b + h);
            if (x) return h + (uint64_t)(__builtin_ctzll(x) >> 3);
            h += 8u;
        } else {
            if (a[h] != b[h]) break;
            ++h;
        }
    }
    return h;
}

__device__ __forceinline__ uint32_t cross_lcp(const MrgSide &r, uint32_t i, const MrgSide &g, uint32_t k, uint32_t lcp_cap)
{
    const Suffix a = suffix_at(r, i), b = suffix_at(g, k);
    uint64_t lim = a.len < b.len ? a.len : b.len;
    if (lcp_cap && lim > lcp_cap) lim = lcp_cap;
    return (uint32_t)match_from(a.sym, b.sym, 0, lim);
}

__global__ void __launch_bounds__(MRG_WG) k_mrg_rank(MrgSide r, MrgSide g, uint32_t *j)
{
    for (uint64_t i = blockIdx.x * (uint64_t)MRG_WG + threadIdx.x; i < r.n; i += (uint64_t)gridDim.x * MRG_WG) {
        const Suffix a = suffix_at(r, (uint32_t)i);
        uint32_t lo = 0, hi = g.n;                                          // genome suffixes below lo are below a, those from hi on above
        uint64_t ml = 0, mh = 0;                                            // symbols a shares with suffix lo - 1 and with suffix hi
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const Suffix b = suffix_at(g, mid);
            const uint64_t lim = a.len < b.len ? a.len : b.len;
            const uint64_t h = match_from(a.sym, b.sym, ml < mh ? ml : mh, lim);
            const bool below = h < lim ? b.sym[h] < a.sym[h] : b.len < a.len;            // ends together: the read is the lower one
            if (below) { lo = mid + 1u; ml = h; } else { hi = mid; mh = h; }
        }
        j[i] = lo;
    }
}

__global__ void __launch_bounds__(MRG_WG) k_mrg_ends(const uint32_t *j, uint32_t nr, uint32_t ng, uint32_t *end, uint32_t *runs)
{
    uint32_t mine = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)MRG_WG + threadIdx.x; i < nr; i += (uint64_t)gridDim.x * MRG_WG) {
        const uint32_t a = j[i];
        if (i + 1u == nr || a != j[i + 1u]) { if (a <= ng) end[a] = (uint32_t)i + 1u; ++mine; }
    }
    if (mine) atomicAdd(runs, mine);
}

__global__ void __launch_bounds__(MRG_WG) k_mrg_write_reads(MrgSide r, MrgSide g, const uint32_t *j, uint32_t lcp_cap, uint8_t *ebwt, uint32_t *lcp, uint32_t *da)
{
    for (uint64_t i = blockIdx.x * (uint64_t)MRG_WG + threadIdx.x; i < r.n; i += (uint64_t)gridDim.x * MRG_WG) {
        const uint32_t ji = j[i] < g.n ? j[i] : g.n;
        const uint64_t slot = i + ji;
        if (da) da[slot] = r.da[i];
        if (ebwt) ebwt[slot] = r.ebwt[i];
        if (!lcp) continue;
        uint32_t v = 0;
        if (i > 0 && j[i - 1u] == j[i]) {                                   // the slot before is read suffix i - 1
            v = r.lcp[i];
            if (lcp_cap && v > lcp_cap) v = lcp_cap;
        } else if (ji > 0) {                                                // the slot before is genome suffix j - 1
            v = cross_lcp(r, (uint32_t)i, g, ji - 1u, lcp_cap);
        }
        lcp[slot] = v;
    }
}

__global__ void __launch_bounds__(MRG_WG) k_mrg_write_genomes(MrgSide r, MrgSide g, const uint32_t *c, uint32_t lcp_cap, uint8_t *ebwt, uint32_t *lcp, uint32_t *da)
{
    for (uint64_t k = blockIdx.x * (uint64_t)MRG_WG + threadIdx.x; k < g.n; k += (uint64_t)gridDim.x * MRG_WG) {
        const uint32_t ck = c[k] < r.n ? c[k] : r.n, before = k ? c[k - 1u] : 0u;
        const uint64_t slot = k + ck;
        if (da) da[slot] = r.n_docs + g.da[k];
        if (ebwt) ebwt[slot] = g.ebwt[k];
        if (!lcp) continue;
        uint32_t v = 0;
        if (c[k] == before) {                                               // no read suffix between genome suffixes k - 1 and k
            v = k ? g.lcp[k] : 0u;
            if (lcp_cap && v > lcp_cap) v = lcp_cap;
        } else if (ck > 0) {                                                // the slot before is read suffix c[k] - 1
            v = cross_lcp(r, ck - 1u, g, (uint32_t)k, lcp_cap);
        }
        lcp[slot] = v;
    }
}

inline uint32_t blocks_for(uint64_t items, uint32_t cap)
{
    const uint64_t b = (items + MRG_WG - 1) / MRG_WG;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

} // namespace

void mrg_launch_rank(const MrgSide &r, const MrgSide &g, uint32_t *j, hipStream_t st)
{
    if (r.n) k_mrg_rank<<<blocks_for(r.n, MRG_RANK_BLOCKS), MRG_WG, 0, st>>>(r, g, j);
}

void mrg_launch_ends(const uint32_t *j, uint32_t nr, uint32_t ng, uint32_t *end, uint32_t *runs, hipStream_t st)
{
    if (nr) k_mrg_ends<<<blocks_for(nr, MRG_ENDS_BLOCKS), MRG_WG, 0, st>>>(j, nr, ng, end, runs);
}

void mrg_launch_write_reads(const MrgSide &r, const MrgSide &g, const uint32_t *j, uint32_t lcp_cap, uint8_t *ebwt, uint32_t *lcp, uint32_t *da, hipStream_t st)
{
    if (r.n) k_mrg_write_reads<<<blocks_for(r.n, MRG_WRITE_BLOCKS), MRG_WG, 0, st>>>(r, g, j, lcp_cap, ebwt, lcp, da);
}

void mrg_launch_write_genomes(const MrgSide &r, const MrgSide &g, const uint32_t *c, uint32_t lcp_cap, uint8_t *ebwt, uint32_t *lcp, uint32_t *da, hipStream_t st)
{
    if (g.n) k_mrg_write_genomes<<<blocks_for(g.n, MRG_WRITE_BLOCKS), MRG_WG, 0, st>>>(r, g, c, lcp_cap, ebwt, lcp, da);
}

} // namespace lime
