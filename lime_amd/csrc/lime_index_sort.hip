// lime_index_sort.hip -- the index builder's key/value sorts and prefix sums: rocPRIM's device primitives, nothing else.
// A translation unit of its own because rocPRIM uses DPP and other cross-lane instructions freely: tools/exec_lint.py and the
// spill gate (`make resources`) look at the project's own kernels (lime_index_kernel.hip), not at these.
#include <cstring>                               // (rocPRIM's texture_cache_iterator.hpp uses memset without it)
#include <rocprim/rocprim.hpp>

#include "lime_index.h"

namespace lime {

hipError_t idx_sort_pairs(void *temp, size_t *temp_bytes, IdxPairs *b, size_t m, unsigned begin_bit, unsigned end_bit, hipStream_t st)
{
    rocprim::double_buffer<uint64_t> k(b->keys[b->cur], b->keys[b->cur ^ 1]);
    rocprim::double_buffer<uint32_t> v(b->vals[b->cur], b->vals[b->cur ^ 1]);
    const hipError_t e = rocprim::radix_sort_pairs(temp, *temp_bytes, k, v, m, begin_bit, end_bit, st);
    if (temp && e == hipSuccess && k.current() != b->keys[b->cur]) b->cur ^= 1;
    return e;
}

hipError_t idx_scan_sum(void *temp, size_t *temp_bytes, const uint32_t *in, uint32_t *out, size_t m, bool inclusive, hipStream_t st)
{
    return inclusive ? rocprim::inclusive_scan(temp, *temp_bytes, in, out, m, rocprim::plus<uint32_t>(), st)
                     : rocprim::exclusive_scan(temp, *temp_bytes, in, out, 0u, m, rocprim::plus<uint32_t>(), st);
}

// the exclusive sum of 64-bit words (the rows' offsets of lime_lists_concat_dev: a list may hold more than 2^32 pairs)
hipError_t idx_scan_sum64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, size_t m, hipStream_t st)
{
    return rocprim::exclusive_scan(temp, *temp_bytes, in, out, (uint64_t)0, m, rocprim::plus<uint64_t>(), st);
}

hipError_t idx_scan_max(void *temp, size_t *temp_bytes, const uint32_t *in, uint32_t *out, size_t m, hipStream_t st)
{
    return rocprim::inclusive_scan(temp, *temp_bytes, in, out, m, rocprim::maximum<uint32_t>(), st);
}

} // namespace lime
