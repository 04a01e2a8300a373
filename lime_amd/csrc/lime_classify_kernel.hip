// lime_classify_kernel.hip -- the read-assignment decision (lime_classify.cpp's decide(); reference: src/Classify.cpp:503-690) on the
// device, over the clusterChoose lists that lime_choose_lists_dev / lime_fused_choose_lists_dev left in HBM (lime_choose.cpp:
// lime_classify_lists_dev).  One wave64 per read, grid-stride over the reads; the lanes stride over the read's rows of the 2 or 4
// lists taken one after the other ("elements": list i, genome g, count k).  Per read, in order, each pass only if the ones before
// decided nothing:
//   A  rule 1: the candidates (elements of the lists whose record top is within TOL of the best top, and whose own value is within
//      TOL of that top); one taxon <=> min == max of their at_rank over the wave.  No searches: the element's own value decides.
//   B  the candidates' per-strand sums (v0 + v3, v1 + v2; v_j by binary search in list j's row, which is sorted by idRef) and the
//      union's sums over all genomes (a genome counts in the first list that holds it): wave maxima top2[2], hi[2].
//   C  rule 2: the candidates whose winning-strand sum equals its maximum: min == max of at_rank.
//   D  rule 3: the genomes within TOL of h: min / max of at_rank and of the higher ranks.  When h < TOL every genome that is in no
//      list (sum 0) is selected too: that read walks all n_targ genomes instead of the union (exact, slow).
// Every float is a table lookup (the host builds the 256 values of each list with the writer's own expression), a float add or a
// compare, in decide()'s order: no division, no multiply (so contraction cannot change a bit).  Cross-lane operations (the wave
// reductions) run only at the read's top level, under wave-uniform conditions made scalar with readfirstlane.
// Two kernels run the one decision: k_classify (a norm per list, the tables in LDS) and k_classify_norms (a norm per list and read,
// lists with per-read norms: the tables in device memory).  A call without per-read lists launches k_classify, as it always did.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_kernels.h"

namespace lime {

namespace {

constexpr float CTOL = static_cast<float>(0.02);      // ERROR, src/Tools.h:37 (lime_classify.h TOL)
constexpr int CLS_WG = 256;                            // 4 independent waves per workgroup

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float unif(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ uint32_t red_min(uint32_t v)
{
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = o < v ? o : v; }
    return uni(v);
}
__device__ __forceinline__ uint32_t red_max(uint32_t v)
{
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    return uni(v);
}
__device__ __forceinline__ float red_maxf(float v)
{
    for (int d = 32; d > 0; d >>= 1) { const float o = __shfl_xor(v, d); if (v < o) v = o; }
    return unif(v);
}

// the lists' 12 pointers, copied from the kernel arguments into LDS at the start: read from there they live in vector registers
// (as kernel arguments they stayed in the scalar file, which then spilled)
struct ListPtrs { const uint8_t *row_max[4]; const uint64_t *row_off[4]; const lime_pair_t *pairs[4]; };

struct ReadRows {                 // one read's rows in the lists (wave-uniform)
    uint64_t b[4];                // first pair of the row
    uint32_t c[5];                // element index where list i starts (c[n_lists..4] = total)
    float top[4];                 // the list's record top (0: no record)
};

// count of genome g in a row of len pairs at P + b, or -1 (binary search over the row's ascending idRef)
__device__ __forceinline__ int find_in(const lime_pair_t *P, uint64_t b, uint32_t len, uint32_t g)
{
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (P[b + mid].id_ref < g) lo = mid + 1; else hi = mid;
    }
    if (lo < len) { const lime_pair_t p = P[b + lo]; if (p.id_ref == g) return (int)(p.sim & 0xFFu); }
    return -1;
}

// Where the floats come from.  The decision is written once over an accessor: val(i, k) the value of count k in list i, top(i, m) the
// record top of a row whose maximum is m (0: no record).
//   TabLds    one norm per list (k_classify): the workgroup's copy in LDS of the lists' tables, [4][2][256].
//   TabNorms  one norm per list AND read (k_classify_norms): the tables stay in device memory, [blocks][256][2][256]; per read the wave
//             leaves in LDS the four addresses of its read's tables (block and norm chosen), and a lookup is one LDS read of the list's
//             address and one load through the vector cache.  Nothing of a table is copied per read, and the scalar file, which
//             k_classify fills, holds nothing more.
struct TabLds {
    const float (*t)[2][256];
    template <typename K> __device__ __forceinline__ float val(uint32_t i, K k) const { return t[i][0][k]; }
    template <typename K> __device__ __forceinline__ float top(uint32_t i, K m) const { return t[i][1][m]; }
};
struct TabNorms {
    const float *const *rowp;                          // LDS: where the tables [2][256] of this wave's read start, one pointer per list
    template <typename K> __device__ __forceinline__ float val(uint32_t i, K k) const { return rowp[i][(uint32_t)k]; }
    template <typename K> __device__ __forceinline__ float top(uint32_t i, K m) const { return rowp[i][256u + (uint32_t)m]; }
};

// the values of genome g in every list (0 where absent); *earlier: g is in a list before `own` (own = 4: none is skipped)
template <typename Tab>
__device__ __forceinline__ void values_of(const ClsArgs &a, const ListPtrs &lp, const ReadRows &R, const Tab tab, uint32_t g, uint32_t own,
                                          float own_v, float v[4], bool *earlier)
{
    bool e = false;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        v[j] = 0.0f;
        if (j >= a.n_lists) continue;                  // (uniform)
        if (j == own) { v[j] = own_v; continue; }
        const int k = find_in(lp.pairs[j], R.b[j], R.c[j + 1] - R.c[j], g);
        if (k >= 0) { v[j] = tab.val(j, k); if (j < own) e = true; }
    }
    *earlier = e;
}

struct Elem { uint32_t i, g, k; };
__device__ __forceinline__ Elem element(const ListPtrs &lp, const ReadRows &R, uint32_t t)
{
    const uint32_t i = (t >= R.c[1]) + (t >= R.c[2]) + (t >= R.c[3]);
    const lime_pair_t *P = lp.pairs[i];
    const uint64_t b = i == 0 ? R.b[0] : i == 1 ? R.b[1] : i == 2 ? R.b[2] : R.b[3];
    const uint32_t c = i == 0 ? R.c[0] : i == 1 ? R.c[1] : i == 2 ? R.c[2] : R.c[3];
    const lime_pair_t p = P[b + (t - c)];
    return Elem{i, p.id_ref, p.sim & 0xFFu};
}
__device__ __forceinline__ float top_of(const ReadRows &R, uint32_t i) { return i == 0 ? R.top[0] : i == 1 ? R.top[1] : i == 2 ? R.top[2] : R.top[3]; }

// per-lane accumulators of the taxa of a selected set: [0] at the chosen rank, [1 + q] higher rank q
struct TaxAcc {
    uint32_t mn[7], mx[7], any;
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int q = 0; q < 7; ++q) { mn[q] = 0xFFFFFFFFu; mx[q] = 0u; }
        any = 0u;
    }
    __device__ __forceinline__ void add(const ClsArgs &a, uint32_t g)
    {
        const uint32_t gi = g < a.n_targ ? g : 0u;     // (an idRef beyond n_targ is an error the host reports; nothing is read out of bounds)
        const uint32_t t = a.at_rank[gi];
        mn[0] = t < mn[0] ? t : mn[0]; mx[0] = t > mx[0] ? t : mx[0];
        any = 1u;
        if (a.higher) {
#pragma unroll
            for (uint32_t q = 0; q < 6; ++q) {
                if (q < a.rank_lo) continue;
                const uint32_t h = a.higher[(size_t)q * a.n_targ + gi];
                mn[q + 1] = h < mn[q + 1] ? h : mn[q + 1]; mx[q + 1] = h > mx[q + 1] ? h : mx[q + 1];
            }
        }
    }
};

__device__ __forceinline__ lime_verdict_t verdict(uint8_t type, uint32_t taxon, float sim, uint8_t rule)
{
    lime_verdict_t v;
    v.taxon = taxon; v.sim = sim; v.type = type; v.rule = rule; v.pad[0] = 0; v.pad[1] = 0;
    return v;
}

__device__ __forceinline__ bool candidate(float best, float ti, float vi) { return ti != 0.0f && best - ti < CTOL && ti - vi < CTOL; }
__device__ __forceinline__ bool selected(uint32_t br, float h, float s0, float s1)
{
    return br == 0u ? (h - s0 < CTOL) : br == 1u ? (h - s1 < CTOL) : ((h - s0 < CTOL) || (h - s1 < CTOL));
}

// the whole decision of read r by one wave; every value it returns is wave-uniform
template <typename Tab>
__device__ __forceinline__ lime_verdict_t classify_read(const ClsArgs &a, const ListPtrs &lp, const Tab tab, uint32_t r)
{
    const uint32_t lane = __lane_id();
    ReadRows R;
    float best = 0.0f;
    bool any = false;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        R.c[i] = c; R.b[i] = 0; R.top[i] = 0.0f;
        if (i >= a.n_lists) continue;
        const uint64_t b = lp.row_off[i][r], e = lp.row_off[i][r + 1];
        R.b[i] = b;
        c += uni((uint32_t)(e - b));
        R.top[i] = unif(tab.top(i, lp.row_max[i][r]));
        if (R.top[i] != 0.0f) { if (!any || R.top[i] > best) best = R.top[i]; any = true; }
    }
    R.c[4] = c;
    const uint32_t T = c;
    if (!any) return verdict('U', 0u, 0.0f, 0);

    // ---- A: rule 1 (the element's own value decides candidacy) ----
    TaxAcc acc;
    acc.init();
    uint32_t bad = 0;
    for (uint32_t base = 0; base < T; base += 64) {
        const uint32_t t = base + lane;
        if (t < T) {
            const Elem el = element(lp, R, t);
            if (el.g >= a.n_targ) bad = 1u;
            if (candidate(best, top_of(R, el.i), tab.val(el.i, el.k))) acc.add(a, el.g);
        }
    }
    if (bad) atomicOr(a.err, 1u);
    {
        const uint32_t n = red_max(acc.any), lo = red_min(acc.mn[0]), hi = red_max(acc.mx[0]);
        if (n && lo == hi) return verdict('C', lo, best, 1);
    }

    // ---- B: the candidates' per-strand maxima, the union's sums' maxima ----
    float t0 = 0.0f, t1 = 0.0f, h0 = 0.0f, h1 = 0.0f;
    for (uint32_t base = 0; base < T; base += 64) {
        const uint32_t t = base + lane;
        if (t < T) {
            const Elem el = element(lp, R, t);
            const float vi = tab.val(el.i, el.k);
            float v[4]; bool earlier;
            values_of(a, lp, R, tab, el.g, el.i, vi, v, &earlier);
            const float s0 = v[0] + v[3], s1 = v[1] + v[2];
            if (candidate(best, top_of(R, el.i), vi)) { if (t0 < s0) t0 = s0; if (t1 < s1) t1 = s1; }
            if (!earlier && el.g < a.n_targ) { if (h0 < s0) h0 = s0; if (h1 < s1) h1 = s1; }
        }
    }
    t0 = red_maxf(t0); t1 = red_maxf(t1); h0 = red_maxf(h0); h1 = red_maxf(h1);

    // ---- C: rule 2 ----
    uint32_t win = 2; float wtop = 0.0f;
    if (t0 > t1 + CTOL) { win = 0; wtop = t0; }
    else if (t1 > t0 + CTOL) { win = 1; wtop = t1; }
    if (win < 2) {
        acc.init();
        for (uint32_t base = 0; base < T; base += 64) {
            const uint32_t t = base + lane;
            if (t < T) {
                const Elem el = element(lp, R, t);
                const float vi = tab.val(el.i, el.k);
                if (candidate(best, top_of(R, el.i), vi)) {
                    float v[4]; bool earlier;
                    values_of(a, lp, R, tab, el.g, el.i, vi, v, &earlier);
                    const float s = win == 0 ? v[0] + v[3] : v[1] + v[2];
                    if (s == wtop) acc.add(a, el.g);
                }
            }
        }
        const uint32_t n = red_max(acc.any), lo = red_min(acc.mn[0]), hi = red_max(acc.mx[0]);
        if (n && lo == hi) return verdict('C', lo, wtop, 2);
    }

    // ---- D: rule 3 over all genomes ----
    const uint32_t br = h0 > h1 ? 0u : h0 < h1 ? 1u : 2u;
    const float h = br == 1u ? h1 : h0;
    acc.init();
    if (h < CTOL) {
        // the genomes in no list (sums 0) are within TOL of h too: every genome is looked at
        for (uint32_t base = 0; base < a.n_targ; base += 64) {
            const uint32_t g = base + lane;
            if (g < a.n_targ) {
                float v[4]; bool earlier;
                values_of(a, lp, R, tab, g, 4u, 0.0f, v, &earlier);
                if (selected(br, h, v[0] + v[3], v[1] + v[2])) acc.add(a, g);
            }
        }
    } else {
        for (uint32_t base = 0; base < T; base += 64) {
            const uint32_t t = base + lane;
            if (t < T) {
                const Elem el = element(lp, R, t);
                float v[4]; bool earlier;
                values_of(a, lp, R, tab, el.g, el.i, tab.val(el.i, el.k), v, &earlier);
                if (!earlier && el.g < a.n_targ && selected(br, h, v[0] + v[3], v[1] + v[2])) acc.add(a, el.g);
            }
        }
    }
    if (!red_max(acc.any)) return verdict('A', 0u, 0.0f, 3);
    {
        const uint32_t lo = red_min(acc.mn[0]), hi = red_max(acc.mx[0]);
        if (lo == hi) return verdict('C', lo, h, 3);
    }
    if (a.higher) {
        for (uint32_t q = a.rank_lo; q < 6; ++q) {
            uint32_t m0 = 0, m1 = 0;                   // (the accumulators of rank q, picked by an unrolled select: they stay in registers)
#pragma unroll
            for (uint32_t z = 0; z < 6; ++z) if (z == q) { m0 = acc.mn[z + 1]; m1 = acc.mx[z + 1]; }
            const uint32_t lo = red_min(m0), hi = red_max(m1);
            if (lo == hi && lo != 0u) return verdict('H', lo, h, 3);
        }
    }
    return verdict('A', 0u, 0.0f, 3);
}

__global__ void __launch_bounds__(CLS_WG) k_classify(ClsArgs a)
{
    __shared__ float tab[4][2][256];                   // per list: the cell values, the record tops
    __shared__ ListPtrs lp;
    for (uint32_t k = threadIdx.x; k < 4u * 2u * 256u; k += CLS_WG) (&tab[0][0][0])[k] = a.tabs[k];
    if (threadIdx.x < 4) { lp.row_max[threadIdx.x] = a.row_max[threadIdx.x]; lp.row_off[threadIdx.x] = a.row_off[threadIdx.x]; lp.pairs[threadIdx.x] = a.pairs[threadIdx.x]; }
    __syncthreads();
    const uint32_t wave = blockIdx.x * (CLS_WG / 64) + uni(threadIdx.x >> 6), n_waves = gridDim.x * (CLS_WG / 64);
    for (uint32_t r = wave; r < a.n_reads; r += n_waves) {
        const lime_verdict_t v = classify_read(a, lp, TabLds{tab}, r);
        if (__lane_id() == 0) a.out[r] = v;
    }
}

// the same decision, every read by the tables of its own norms; the lists' and the norms' pointers go through LDS like k_classify's
__global__ void __launch_bounds__(CLS_WG) k_classify_norms(ClsNormArgs n)
{
    __shared__ ListPtrs lp;
    __shared__ const uint8_t *np[4];
    __shared__ const float *bp[4];                     // per list: its block of 256 tables
    __shared__ lime_verdict_t *outp;
    if (threadIdx.x == 0) outp = n.a.out;
    __shared__ const float *rowp[CLS_WG / 64][4];      // per wave: its read's tables
    if (threadIdx.x < 4) {
        lp.row_max[threadIdx.x] = n.a.row_max[threadIdx.x]; lp.row_off[threadIdx.x] = n.a.row_off[threadIdx.x]; lp.pairs[threadIdx.x] = n.a.pairs[threadIdx.x];
        np[threadIdx.x] = n.norms[threadIdx.x];        // (NULL for a list with one norm, and behind the last list)
        bp[threadIdx.x] = n.a.tabs + ((size_t)((n.block >> (8u * threadIdx.x)) & 0xFFu) << 17);
    }
    __syncthreads();
    const uint32_t w = uni(threadIdx.x >> 6), lane = __lane_id();
    const uint32_t wave = blockIdx.x * (CLS_WG / 64) + w, n_waves = gridDim.x * (CLS_WG / 64);
    TabNorms tab;
    tab.rowp = rowp[w];
    for (uint32_t r = wave; r < n.a.n_reads; r += n_waves) {
        // lanes 0 .. 3 write the addresses, every lane reads them: one wave, whose LDS operations keep their order
        __builtin_amdgcn_wave_barrier();
        if (lane < 4) {
            const uint8_t *p = np[lane];
            rowp[w][lane] = bp[lane] + ((size_t)(p ? (uint32_t)p[r] : 0u) << 9);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const lime_verdict_t v = classify_read(n.a, lp, tab, r);
        if (lane == 0) outp[r] = v;
    }
}

} // namespace

void launch_classify_norms(const ClsNormArgs &a, hipStream_t st)
{
    if (!a.a.n_reads) return;
    const uint32_t waves = CLS_WG / 64;
    uint64_t blocks = ((uint64_t)a.a.n_reads + waves - 1) / waves;
    if (blocks > 4096) blocks = 4096;                  // as launch_classify
    hipLaunchKernelGGL(k_classify_norms, dim3((uint32_t)blocks), dim3(CLS_WG), 0, st, a);
}

void launch_classify(const ClsArgs &a, hipStream_t st)
{
    if (!a.n_reads) return;
    const uint32_t waves = CLS_WG / 64;
    uint64_t blocks = ((uint64_t)a.n_reads + waves - 1) / waves;
    if (blocks > 4096) blocks = 4096;                  // 16 workgroups per CU of 256 CUs; the rest by grid stride
    hipLaunchKernelGGL(k_classify, dim3((uint32_t)blocks), dim3(CLS_WG), 0, st, a);
}

} // namespace lime
