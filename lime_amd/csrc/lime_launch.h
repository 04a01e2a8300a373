// lime_launch.h -- host-side helpers of the launch wrappers in the kernel family files: the device index their per-device caches
// are keyed by, the resident-workgroup query, and the preload hooks of the family files (launch_preload, lime_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lime {

template <typename K> static inline uint32_t resident_blocks(K kernel, int block)
{
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 1024u;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    return (uint32_t)per_cu * (uint32_t)prop.multiProcessorCount;
}

// per-device caches of the launch wrappers (one process may drive several GPUs from several host threads)
constexpr int MAX_DEV = 64;
static inline int cur_device() { int d = 0; (void)hipGetDevice(&d); return d >= 0 && d < MAX_DEV ? d : 0; }

// launch_preload: a family file loads the code of its own kernels and fills its wrappers' per-device caches
template <typename K> static inline void preload_kernel(K kernel)
{
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(kernel));
}
void preload_partition();
void preload_apply();

} // namespace lime
