// lime_listcat_kernel.hip -- clusterChoose lists of column shards of one table made into the whole table's list (lime_choose.cpp:
// lime_lists_concat_dev sequences the passes; include/lime_hip.h states the contract).  The parts are P >= 1 lists over the same
// n_reads rows, each with row_max u8[n_reads], row_off u64[n_reads + 1] and pairs ascending by idRef inside a row, made with a test
// every non-zero row passes; part p's genomes are the whole table's columns id_base[p] .. (id_base ascending and the parts' id ranges
// apart: checked by the host).  A row of the whole table is its parts' rows one after the other, and clusterChoose's test
// (ClusterBWT_DA.cpp:404-406) is taken on the maximum over the parts: a row passes as a whole or not at all.
//   k_lc_rows  one lane per read, grid-stride: row_max[r] = the maximum over the parts, len[r] = the sum of the parts' row lengths
//              where pass[row_max[r]], else 0; len[n_reads] = 0.  pass is the host's table of the reference's test for the 256 values a
//              maximum takes: nothing is divided here.
//   (one exclusive prefix sum of len over n_reads + 1 entries, rocPRIM in lime_index_sort.hip: the output's row_off, and the total)
//   k_lc_copy  one wave64 per read (a workgroup is one wave), grid-stride: the pairs of a row that passes, part after part, the lanes
//              striding over a part's row, id_ref + id_base[p], sim as it is.  Ascending idRef is kept by construction.
// The parts' table (LcPart[P]) lives in device memory and is read with wave-uniform indices: P is not bounded by a kernel argument.
// A part without pairs has a NULL pairs pointer: all its rows are empty, so it is never dereferenced.  No store goes outside the
// output's row ([row_off[r], row_off[r + 1]) of the pairs, entry r of row_max and len), no load outside the parts' blocks.  The only
// cross-lane operation is readfirstlane on the wave's number, at the kernel's top level.  No inline assembly, plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lime_kernels.h"

namespace lime {

namespace {

constexpr int LC_ROWS_WG = 256;
constexpr int LC_COPY_WG = 64;                   // one wave per workgroup: 8192 workgroups are the waves the device holds at once
constexpr uint32_t LC_BLOCKS = 8192;             // grids are capped and both kernels stride

__global__ void __launch_bounds__(LC_ROWS_WG) k_lc_rows(const LcPart *parts, uint32_t n_parts, uint32_t n_reads, const uint8_t *pass,
                                                         uint8_t *row_max, unsigned long long *len)
{
    const uint64_t stride = (uint64_t)gridDim.x * LC_ROWS_WG;
    for (uint64_t r = (uint64_t)blockIdx.x * LC_ROWS_WG + threadIdx.x; r < n_reads; r += stride) {
        uint32_t mx = 0u;
        uint64_t sum = 0;
        for (uint32_t p = 0; p < n_parts; ++p) {
            const LcPart q = parts[p];
            const uint32_t m = q.row_max[r];
            mx = m > mx ? m : mx;
            sum += q.row_off[r + 1] - q.row_off[r];
        }
        row_max[r] = (uint8_t)mx;
        len[r] = pass[mx] ? sum : 0ull;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len[n_reads] = 0ull;
}

__global__ void __launch_bounds__(LC_COPY_WG) k_lc_copy(const LcPart *parts, uint32_t n_parts, uint32_t n_reads, const uint64_t *row_off,
                                                         lime_pair_t *out)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)blockIdx.x);      // (the wave's number: scalar, so are the rows' bounds)
    for (uint64_t r = first; r < n_reads; r += gridDim.x) {
        uint64_t dst = row_off[r];
        const uint64_t end = row_off[r + 1];
        if (dst == end) continue;                // a row that does not pass, or holds nothing
        for (uint32_t p = 0; p < n_parts; ++p) {
            const LcPart q = parts[p];
            const uint64_t b = q.row_off[r], n = q.row_off[r + 1] - b;
            for (uint64_t i = lane; i < n && dst + i < end; i += LC_COPY_WG) {
                lime_pair_t v = q.pairs[b + i];
                v.id_ref += q.id_base;
                out[dst + i] = v;
            }
            dst += n;
        }
    }
}

} // namespace

void launch_lc_rows(const LcPart *parts, uint32_t n_parts, uint32_t n_reads, const uint8_t *pass, uint8_t *row_max, uint64_t *len, hipStream_t st)
{
    const uint64_t want = ((uint64_t)n_reads + LC_ROWS_WG - 1) / LC_ROWS_WG;
    const uint32_t grid = want < LC_BLOCKS ? (want ? (uint32_t)want : 1u) : LC_BLOCKS;      // (n_reads == 0: one workgroup writes len[0])
    k_lc_rows<<<grid, LC_ROWS_WG, 0, st>>>(parts, n_parts, n_reads, pass, row_max, (unsigned long long *)len);
}

void launch_lc_copy(const LcPart *parts, uint32_t n_parts, uint32_t n_reads, const uint64_t *row_off, lime_pair_t *out, hipStream_t st)
{
    if (!n_reads) return;
    k_lc_copy<<<n_reads < LC_BLOCKS ? n_reads : LC_BLOCKS, LC_COPY_WG, 0, st>>>(parts, n_parts, n_reads, row_off, out);
}

} // namespace lime
