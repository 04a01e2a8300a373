// lime_readnorm_kernel.hip -- every read normalised by its own length (lime_docs.cpp: lime_docs_norms_dev,
// lime_choose.cpp: lime_lists_concat_norms_dev; include/lime_hip.h states the contracts).  The reference divides every read's counts by
// one norm = readLen + 1 - alpha (ClusterBWT_DA.cpp:555, :404); here the norm of read r comes from its own length, which is already in
// HBM as doc_off of its lime_docs.
//   k_rn_norms  one lane per read, grid-stride over doc_off[n_docs + 1]: len = doc_off[r + 1] - doc_off[r], norm[r] = len + 1 - alpha
//               where len >= alpha, else 1 (such a read is in no alpha-cluster: its rows are empty whatever the norm), stored as u8.
//               A read of more than 255 symbols has no norm a byte holds (and none --readlen could name): such reads are counted
//               in info[0] and the lowest of their indices is left in info[1] by a 32-bit atomic min; their norm byte is 0.
//   k_rn_rows   k_lc_rows (lime_listcat_kernel.hip) with clusterChoose's test taken per read: pass[norm[r]][row_max[r]] instead of
//               pass[row_max[r]].  pass is the host's 256 x 256 table, row n the reference's test for norm n in the reference's types
//               (row 0 all false): nothing is divided here.  The prefix sum and k_lc_copy that follow are the fixed-norm path's own.
// No store goes outside norm[0 .. n_docs), info[0 .. 2), row_max[0 .. n_reads) and len[0 .. n_reads]; no load outside doc_off[0 .. n_docs],
// norm[0 .. n_reads), the 64 KB of pass and the parts' blocks.  No cross-lane operation, no inline assembly, plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_kernels.h"

namespace lime {

namespace {

constexpr int RN_WG = 256;
constexpr uint32_t RN_BLOCKS = 1024;             // k_rn_norms: four workgroups per CU; the rest by grid stride
constexpr uint32_t RN_ROWS_BLOCKS = 8192;        // k_rn_rows: k_lc_rows' cap

__global__ void __launch_bounds__(RN_WG) k_rn_norms(const uint64_t *doc_off, uint32_t n_docs, uint32_t alpha, uint8_t *norm, uint32_t *info)
{
    const uint64_t stride = (uint64_t)gridDim.x * RN_WG;
    for (uint64_t r = (uint64_t)blockIdx.x * RN_WG + threadIdx.x; r < n_docs; r += stride) {
        const uint64_t len = doc_off[r + 1] - doc_off[r];
        uint32_t v;
        if (len > 255u) {
            v = 0u;
            atomicAdd(&info[0], 1u);
            atomicMin(&info[1], (uint32_t)r);
        } else {
            v = len >= alpha ? (uint32_t)len + 1u - alpha : 1u;
        }
        norm[r] = (uint8_t)v;
    }
}

__global__ void __launch_bounds__(RN_WG) k_rn_rows(const LcPart *parts, uint32_t n_parts, uint32_t n_reads, const uint8_t *norm, const uint8_t *pass,
                                                    uint8_t *row_max, unsigned long long *len)
{
    const uint64_t stride = (uint64_t)gridDim.x * RN_WG;
    for (uint64_t r = (uint64_t)blockIdx.x * RN_WG + threadIdx.x; r < n_reads; r += stride) {
        uint32_t mx = 0u;
        uint64_t sum = 0;
        for (uint32_t p = 0; p < n_parts; ++p) {
            const LcPart q = parts[p];
            const uint32_t m = q.row_max[r];
            mx = m > mx ? m : mx;
            sum += q.row_off[r + 1] - q.row_off[r];
        }
        row_max[r] = (uint8_t)mx;
        len[r] = pass[(uint32_t)norm[r] * 256u + mx] ? sum : 0ull;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len[n_reads] = 0ull;
}

} // namespace

uint32_t rn_norms_lanes() { return RN_BLOCKS * (uint32_t)RN_WG; }

void launch_rn_norms(const uint64_t *doc_off, uint32_t n_docs, uint32_t alpha, uint8_t *norm, uint32_t *info, hipStream_t st)
{
    if (!n_docs) return;
    const uint64_t want = ((uint64_t)n_docs + RN_WG - 1) / RN_WG;
    k_rn_norms<<<want < RN_BLOCKS ? (uint32_t)want : RN_BLOCKS, RN_WG, 0, st>>>(doc_off, n_docs, alpha, norm, info);
}

void launch_rn_rows(const LcPart *parts, uint32_t n_parts, uint32_t n_reads, const uint8_t *norm, const uint8_t *pass, uint8_t *row_max, uint64_t *len,
                    hipStream_t st)
{
    const uint64_t want = ((uint64_t)n_reads + RN_WG - 1) / RN_WG;
    const uint32_t grid = want < RN_ROWS_BLOCKS ? (want ? (uint32_t)want : 1u) : RN_ROWS_BLOCKS;      // (n_reads == 0: one workgroup writes len[0])
    k_rn_rows<<<grid, RN_WG, 0, st>>>(parts, n_parts, n_reads, norm, pass, row_max, (unsigned long long *)len);
}

} // namespace lime
