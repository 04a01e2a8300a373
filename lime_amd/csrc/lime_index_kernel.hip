// lime_index_kernel.hip -- the project's own kernels of the index builder (lime_build_index_dev, lime_build.cpp): ebwt / lcp / da of
// reads + genomes by a generalized suffix sort on the device, in the convention of lime_amd/builder.py (every document followed by
// its own terminator; a terminator sorts below every symbol, two terminators by document id; lcp counts non-terminator symbols).
//   1  k_idx_check / k_idx_present / k_idx_codes   doc_off is checked, the bytes that occur get dense codes 1 .. sigma (0 = terminator)
//   2  k_idx_doc_heads (+ a prefix sum)            the document of every position
//   3  k_idx_pack                                  the first K codes of every suffix in one 64-bit key; a stable sort of (key, position)
//      orders suffixes that reach their terminator inside the window by document id, because positions ascend with the document
//   4  k_idx_heads / k_idx_settle / k_idx_compact  groups of equal keys get their first slot as rank, groups of one are final and leave
//   5  k_idx_double                                the rest sorts by (rank[p], rank[p + h]), h doubling: back to 4 until nothing is left.
//      A suffix that is still in a group after a round of depth h has h real symbols in front of its terminator (one whose terminator
//      is nearer is alone by then), so p + h stays inside p's document.
//   6  k_idx_gather, k_idx_lcp                     da, ebwt; lcp by Kasai's bound over stretches of IDX_STRETCH consecutive positions
// The sorts and prefix sums between them are rocPRIM's (lime_index_sort.hip).  wave64, no cross-lane operation, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_index.h"

namespace lime {

namespace {

constexpr int IDX_WG = 256;
constexpr uint32_t PACK_CHUNKS = 20;             // 16-byte pieces of text one k_idx_pack workgroup stages: 255 + 32 symbols + 15 of alignment

__device__ __forceinline__ uint32_t gtid() { return blockIdx.x * (uint32_t)IDX_WG + threadIdx.x; }

// the 16 bytes at the 16-byte aligned address c; bytes outside [lo, hi) read as 0 and are not touched
__device__ __forceinline__ uint4 load16_within(uintptr_t c, uintptr_t lo, uintptr_t hi)
{
    if (c >= lo && c + 16u <= hi) return *reinterpret_cast<const uint4 *>(c);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < 16u; ++k) {
        const uintptr_t a = c + k;
        const uint32_t b = (a >= lo && a < hi) ? *reinterpret_cast<const uint8_t *>(a) : 0u;
        w[k >> 2] |= b << ((k & 3u) * 8u);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void __launch_bounds__(IDX_WG) k_idx_check(const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, uint32_t *err)
{
    bool bad = false;
    for (uint64_t k = gtid(); k <= n_docs; k += (uint64_t)gridDim.x * IDX_WG) {
        const uint64_t a = doc_off[k];
        if (k == 0 && a != 0) bad = true;
        if (k == n_docs ? a != n_text : a > doc_off[k + 1]) bad = true;
        if (a > n_text) bad = true;
    }
    if (bad) *err = 1u;
}

__global__ void __launch_bounds__(IDX_WG) k_idx_present(const uint8_t *text, uint64_t n_text, uint32_t *present)
{
    __shared__ uint32_t seen[256];
    seen[threadIdx.x] = 0u;
    __syncthreads();
    const uintptr_t lo = (uintptr_t)text, hi = lo + n_text, base = lo & ~(uintptr_t)15;
    const uint64_t n_chunks = (hi - base + 15u) / 16u;
    for (uint64_t i = gtid(); i < n_chunks; i += (uint64_t)gridDim.x * IDX_WG) {
        const uintptr_t c = base + i * 16u;
        const uint4 v = load16_within(c, lo, hi);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t k = 0; k < 16u; ++k)
            if (c + k >= lo && c + k < hi) seen[(w[k >> 2] >> ((k & 3u) * 8u)) & 255u] = 1u;
    }
    __syncthreads();
    if (seen[threadIdx.x]) present[threadIdx.x] = 1u;
}

__global__ void __launch_bounds__(IDX_WG) k_idx_codes(const uint32_t *present, uint16_t *code, uint32_t *sigma)
{
    __shared__ uint32_t seen[256];
    seen[threadIdx.x] = present[threadIdx.x] ? 1u : 0u;
    __syncthreads();
    uint32_t below = 0;
    for (uint32_t b = 0; b < threadIdx.x; ++b) below += seen[b];
    code[threadIdx.x] = seen[threadIdx.x] ? (uint16_t)(below + 1u) : (uint16_t)0;
    if (threadIdx.x == 255u) *sigma = below + seen[255];
}

__global__ void __launch_bounds__(IDX_WG) k_idx_doc_heads(const uint64_t *doc_off, uint32_t n_docs, uint32_t *flags)
{
    for (uint64_t k = (uint64_t)gtid() + 1u; k < n_docs; k += (uint64_t)gridDim.x * IDX_WG) flags[doc_off[k] + k] = 1u;
}

__global__ void __launch_bounds__(IDX_WG) k_idx_pack(IdxText t, const uint16_t *code, uint32_t k_syms, uint32_t bits, uint64_t *keys, uint32_t *vals)
{
    __shared__ uint4 tile[PACK_CHUNKS];
    __shared__ uint16_t s_code[256];
    s_code[threadIdx.x] = code[threadIdx.x];
    // the text this workgroup's positions can touch: p - doc_of[p] never decreases with p and grows by at most 1 per position
    const uint32_t p0 = blockIdx.x * (uint32_t)IDX_WG;
    const uint32_t pl = (t.n - p0 > (uint32_t)IDX_WG) ? p0 + (uint32_t)IDX_WG - 1u : t.n - 1u;
    const uint64_t src_lo = (uint64_t)p0 - t.doc_of[p0];
    uint64_t src_hi = (uint64_t)pl - t.doc_of[pl] + k_syms;
    if (src_hi > t.n_text) src_hi = t.n_text;
    const uintptr_t lo = (uintptr_t)t.text, hi = lo + t.n_text;
    const uintptr_t first = lo + src_lo, base = first & ~(uintptr_t)15;
    const uint32_t off0 = (uint32_t)(first - base);
    const uint32_t n_chunks = src_hi > src_lo ? (uint32_t)((off0 + (src_hi - src_lo) + 15u) / 16u) : 0u;      // <= PACK_CHUNKS
    if (threadIdx.x < n_chunks && threadIdx.x < PACK_CHUNKS) tile[threadIdx.x] = load16_within(base + threadIdx.x * 16u, lo, hi);
    __syncthreads();
    const uint32_t p = p0 + threadIdx.x;
    if (p > pl) return;
    const uint32_t k = t.doc_of[p];
    const uint64_t rem = t.doc_off[k + 1] + k - p;                              // symbols in front of the terminator
    const uint32_t at = off0 + (uint32_t)((uint64_t)p - k - src_lo);
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(tile);
    uint64_t key = 0;
    for (uint32_t j = 0; j < k_syms; ++j) {
        const uint32_t q = at + j;
        const uint32_t c = (j < rem && q < PACK_CHUNKS * 16u) ? s_code[bytes[q]] : 0u;
        key = (key << bits) | c;
    }
    keys[p] = key;
    vals[p] = p;
}

__device__ __forceinline__ bool is_head(const uint64_t *keys, uint32_t j, uint64_t low_mask)
{
    if (j == 0u) return true;
    const uint64_t a = keys[j];
    return a != keys[j - 1] || (low_mask != 0u && (a & low_mask) == 0u);
}

__global__ void __launch_bounds__(IDX_WG) k_idx_heads(const uint64_t *keys, const uint32_t *idx, uint32_t m, uint64_t low_mask, uint32_t *head_pos)
{
    const uint32_t j = gtid();
    if (j >= m) return;
    head_pos[j] = is_head(keys, j, low_mask) ? (idx ? idx[j] : j) : 0u;
}

__global__ void __launch_bounds__(IDX_WG) k_idx_settle(const uint64_t *keys, const uint32_t *vals, const uint32_t *idx, const uint32_t *grp, uint32_t m,
                                                       uint64_t low_mask, uint32_t n, uint32_t *rank, uint32_t *sa, uint32_t *act)
{
    const uint32_t j = gtid();
    if (j >= m) return;
    const bool alone = is_head(keys, j, low_mask) && (j + 1u == m || is_head(keys, j + 1u, low_mask));
    const uint32_t v = vals[j], slot = idx ? idx[j] : j;
    if (v < n && slot < n) { rank[v] = grp[j]; sa[slot] = v; }
    act[j] = alone ? 0u : 1u;
}

__global__ void __launch_bounds__(IDX_WG) k_idx_compact(const uint32_t *vals, const uint32_t *idx, const uint32_t *act, const uint32_t *pos, uint32_t m,
                                                        uint32_t *vals_out, uint32_t *idx_out)
{
    const uint32_t j = gtid();
    if (j >= m || !act[j]) return;
    const uint32_t o = pos[j];
    if (o >= m) return;
    vals_out[o] = vals[j];
    idx_out[o] = idx ? idx[j] : j;
}

__global__ void __launch_bounds__(IDX_WG) k_idx_double(const uint32_t *vals, uint32_t m, const uint32_t *rank, uint32_t n, uint64_t h, uint32_t nb, uint64_t *keys)
{
    const uint32_t j = gtid();
    if (j >= m) return;
    const uint32_t v = vals[j] < n ? vals[j] : n - 1u;
    const uint64_t q = (uint64_t)v + h;
    keys[j] = ((uint64_t)rank[v] << nb) | rank[q < n ? q : n - 1u];
}

__global__ void __launch_bounds__(IDX_WG) k_idx_gather(IdxText t, const uint32_t *sa, uint8_t term, uint32_t *da, uint8_t *ebwt)
{
    const uint32_t i = gtid();
    if (i >= t.n) return;
    const uint32_t p = sa[i] < t.n ? sa[i] : t.n - 1u;
    const uint32_t k = t.doc_of[p];
    if (da) da[i] = k;
    if (ebwt) ebwt[i] = ((uint64_t)p == t.doc_off[k] + k) ? term : t.text[(uint64_t)p - 1u - k];
}

__device__ __forceinline__ uint64_t load8(const uint8_t *p)
{
    uint64_t x;
    __builtin_memcpy(&x, p, 8);
    return x;
}

__global__ void __launch_bounds__(IDX_WG) k_idx_lcp(IdxText t, const uint32_t *sa, const uint32_t *rank, uint32_t lcp_cap, uint32_t *lcp)
{
    const uint64_t first = (uint64_t)gtid() * IDX_STRETCH;
    if (first >= t.n) return;
    const uint64_t last = first + IDX_STRETCH < t.n ? first + IDX_STRETCH : t.n;
    uint32_t kp = t.doc_of[first];
    uint64_t end_p = t.doc_off[kp + 1] + kp;                                    // p's terminator
    uint64_t h = 0;
    for (uint64_t p = first; p < last; ++p) {
        const uint32_t r = rank[p];
        if (r == 0u || r >= t.n) {
            if (r == 0u) lcp[0] = 0u;
            h = 0;
        } else {
            const uint32_t q = sa[r - 1u] < t.n ? sa[r - 1u] : t.n - 1u;
            const uint32_t kq = t.doc_of[q];
            const uint64_t rem_p = end_p - p, rem_q = t.doc_off[kq + 1] + kq - q;
            uint64_t lim = rem_p < rem_q ? rem_p : rem_q;
            if (lcp_cap && lim > lcp_cap) lim = lcp_cap;
            const uint8_t *a = t.text + (p - kp), *b = t.text + ((uint64_t)q - kq);
            if (h > lim) h = lim;
            while (h < lim) {
                if (h + 8u <= lim) {                                            // eight symbols at a time (both stay in front of their terminators)
                    const uint64_t x = load8(a + h) ^ load8(b + h);
                    if (x) { h += (uint64_t)(__builtin_ctzll(x) >> 3); break; }
                    h += 8u;
                } else {
                    if (a[h] != b[h]) break;
                    ++h;
                }
            }
            lcp[r] = (uint32_t)h;
            if (h) --h;
        }
        if (p == end_p && kp + 1u < t.n_docs) { ++kp; end_p = t.doc_off[kp + 1] + kp; h = 0; }
    }
}

inline uint32_t blocks_for(uint64_t items, uint32_t cap = 0x7FFFFFFFu)
{
    const uint64_t b = (items + IDX_WG - 1) / IDX_WG;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

} // namespace

void idx_launch_check(const uint64_t *doc_off, uint32_t n_docs, uint64_t n_text, const uint8_t *text, uint32_t *present, uint32_t *err, hipStream_t st)
{
    k_idx_check<<<blocks_for((uint64_t)n_docs + 1u, 4096u), IDX_WG, 0, st>>>(doc_off, n_docs, n_text, err);
    if (n_text) k_idx_present<<<blocks_for((n_text + 15u) / 16u + 1u, 8192u), IDX_WG, 0, st>>>(text, n_text, present);
}

void idx_launch_codes(const uint32_t *present, uint16_t *code, uint32_t *sigma, hipStream_t st)
{
    k_idx_codes<<<1, IDX_WG, 0, st>>>(present, code, sigma);
}

void idx_launch_doc_heads(const uint64_t *doc_off, uint32_t n_docs, uint32_t *flags, hipStream_t st)
{
    if (n_docs > 1u) k_idx_doc_heads<<<blocks_for(n_docs - 1u, 8192u), IDX_WG, 0, st>>>(doc_off, n_docs, flags);
}

void idx_launch_pack(const IdxText &t, const uint16_t *code, uint32_t k_syms, uint32_t bits, uint64_t *keys, uint32_t *vals, hipStream_t st)
{
    k_idx_pack<<<blocks_for(t.n), IDX_WG, 0, st>>>(t, code, k_syms, bits, keys, vals);
}

void idx_launch_heads(const uint64_t *keys, const uint32_t *idx, uint32_t m, uint64_t low_mask, uint32_t *head_pos, hipStream_t st)
{
    k_idx_heads<<<blocks_for(m), IDX_WG, 0, st>>>(keys, idx, m, low_mask, head_pos);
}

void idx_launch_settle(const uint64_t *keys, const uint32_t *vals, const uint32_t *idx, const uint32_t *grp, uint32_t m, uint64_t low_mask,
                       uint32_t n, uint32_t *rank, uint32_t *sa, uint32_t *act, hipStream_t st)
{
    k_idx_settle<<<blocks_for(m), IDX_WG, 0, st>>>(keys, vals, idx, grp, m, low_mask, n, rank, sa, act);
}

void idx_launch_compact(const uint32_t *vals, const uint32_t *idx, const uint32_t *act, const uint32_t *pos, uint32_t m,
                        uint32_t *vals_out, uint32_t *idx_out, hipStream_t st)
{
    k_idx_compact<<<blocks_for(m), IDX_WG, 0, st>>>(vals, idx, act, pos, m, vals_out, idx_out);
}

void idx_launch_double(const uint32_t *vals, uint32_t m, const uint32_t *rank, uint32_t n, uint64_t h, uint32_t nb, uint64_t *keys, hipStream_t st)
{
    k_idx_double<<<blocks_for(m), IDX_WG, 0, st>>>(vals, m, rank, n, h, nb, keys);
}

void idx_launch_gather(const IdxText &t, const uint32_t *sa, uint8_t term, uint32_t *da, uint8_t *ebwt, hipStream_t st)
{
    k_idx_gather<<<blocks_for(t.n), IDX_WG, 0, st>>>(t, sa, term, da, ebwt);
}

void idx_launch_lcp(const IdxText &t, const uint32_t *sa, const uint32_t *rank, uint32_t lcp_cap, uint32_t *lcp, hipStream_t st)
{
    k_idx_lcp<<<blocks_for(((uint64_t)t.n + IDX_STRETCH - 1u) / IDX_STRETCH), IDX_WG, 0, st>>>(t, sa, rank, lcp_cap, lcp);
}

} // namespace lime
