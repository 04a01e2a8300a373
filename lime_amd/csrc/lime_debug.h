// lime_debug.h -- the macros and globals of the debug / timing builds (-DLIME_ABLATE_BUILD, -DLIME_PHASE_TIMING, -DLIME_MARK,
// -DLIME_WALL_TIMING, -DLIME_PART_TIMING, -DLIME_SORT_TIMING, -DLIME_APPLY_TIMING; make EXTRA=-D...).  In a release build every macro
// here is empty and nothing is defined.  The kernel families are separate translation units without relocatable device code, so a
// debug build's __device__ global and its extern "C" reader are defined in ONE of them: the family file that writes the global
// names itself (LIME_DEBUG_TU_SCAN in lime_kernels.hip / _PARTITION / _APPLY) before it includes this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// timing experiments (tools/quick.sh): a build with -DLIME_ABLATE_BUILD cuts the scan after phase k when the
// environment says LIME_ABLATE=k (results invalid); the release library has no such switch
#ifdef LIME_ABLATE_BUILD
#define ABL(k) (a.ablate == (k))
#else
#define ABL(k) false
#endif

#if defined(LIME_WALL_TIMING) && defined(LIME_DEBUG_TU_SCAN)      // debug build: start and end wall clock (100 MHz) of every wave of the last scan
namespace lime {
__device__ uint64_t g_wall[2 * 8192];
extern "C" int lime_debug_wall(uint64_t *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wall), sizeof(g_wall)); }
__device__ uint32_t g_winmark[1u << 20];       // which wave (+ 1) took window w of the last scan
extern "C" int lime_debug_winmark(uint32_t *out)
{
    int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_winmark), sizeof(g_winmark));
    void *p = nullptr; (void)hipGetSymbolAddress(&p, HIP_SYMBOL(g_winmark)); (void)hipMemset(p, 0, sizeof(g_winmark));
    return rc;
}
} // namespace lime
#endif
#ifdef LIME_PHASE_TIMING     // debug build: per-wave cycle counts of the scan's phases, printed by a few waves
#define PT_DECL uint64_t pt_t = __builtin_readcyclecounter(), pt_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt_m[4] = {0, 0, 0, 0}; uint32_t pt_nwin = 0;
#define PT(i) { const uint64_t n_ = __builtin_readcyclecounter(); pt_acc[i] += n_ - pt_t; pt_t = n_; }
#define PT_WAITVM asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#elif defined(LIME_MARK)     // ISA reading aid: phase borders as comments in the assembly (tools/isa_count.py)
#define PT_DECL
#define PT(i) asm volatile("; LIMEMARK " #i);
#define PT_WAITVM
#else
#define PT_DECL
#define PT(i)
#define PT_WAITVM
#endif

// debug builds: cycles of k_part's / k_part_lines' (LIME_PART_TIMING), k_sort_tiles' (LIME_SORT_TIMING) or k_apply_tiles' (LIME_APPLY_TIMING)
// phases, summed over one wave of every workgroup (tools/part_phases.py).  g_part_pt is one array with one reader: the partition
// kernels' build and the apply kernel's are two builds.
#if (defined(LIME_PART_TIMING) || defined(LIME_SORT_TIMING)) && defined(LIME_APPLY_TIMING)
#error "LIME_APPLY_TIMING and LIME_PART_TIMING / LIME_SORT_TIMING share g_part_pt: one of them per build"
#endif
#if defined(LIME_PART_TIMING) || defined(LIME_APPLY_TIMING) || defined(LIME_SORT_TIMING)
#if ((defined(LIME_PART_TIMING) || defined(LIME_SORT_TIMING)) && defined(LIME_DEBUG_TU_PARTITION)) || (defined(LIME_APPLY_TIMING) && defined(LIME_DEBUG_TU_APPLY))
namespace lime {
__device__ unsigned long long g_part_pt[8];
extern "C" int lime_debug_part_times(unsigned long long *out)
{
    int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_part_pt), sizeof(g_part_pt));
    void *p = nullptr; (void)hipGetSymbolAddress(&p, HIP_SYMBOL(g_part_pt)); (void)hipMemset(p, 0, sizeof(g_part_pt));
    return rc;
}
} // namespace lime
#endif
#define PT_DECL_ uint64_t pp_t = __builtin_readcyclecounter(), pp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PT_(i) { const uint64_t n_ = __builtin_readcyclecounter(); pp_acc[i] += n_ - pp_t; pp_t = n_; }
#ifndef LIME_PT_WAVE
#define LIME_PT_WAVE 0               // the wave of every workgroup whose cycles are summed (tools/r04_part_phases_waves.sh)
#endif
#define PT_END_ if (threadIdx.x == 64 * LIME_PT_WAVE) { for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_part_pt[i_], (unsigned long long)pp_acc[i_]); }
#endif
#ifdef LIME_PART_TIMING
#define PP_DECL PT_DECL_
#define PP(i) PT_(i)
#define PP_END PT_END_
#else
#define PP_DECL
#define PP(i)
#define PP_END
#endif
#ifdef LIME_SORT_TIMING
#define ST_DECL PT_DECL_
#define ST(i) PT_(i)
#define ST_END PT_END_
#define ST_WAITVM asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
#define ST_DECL
#define ST(i)
#define ST_END
#define ST_WAITVM
#endif
#ifdef LIME_APPLY_TIMING
#define AP_DECL PT_DECL_
#define AP(i) PT_(i)
#define AP_END PT_END_
#define AP_WAITVM asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
#define AP_DECL
#define AP(i)
#define AP_END
#define AP_WAITVM
#endif
