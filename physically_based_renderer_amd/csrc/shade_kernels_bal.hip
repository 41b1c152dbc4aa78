// shade_kernels_bal.hip -- the wave-balanced point-light kernels (shade_tile_kernel BAL 1 and 2, pbr_balanced.h)
// in a translation unit of their own: the Makefile builds shade_kernels.hip with the max-ILP machine scheduler (faster
// for the uniform and culled loops, no scratch) and this unit with the default scheduler (max-ILP spills 12-44 B/lane
// in the balanced kernels). Development builds (PBR_BAL_PROFILE, PBR_WAVE_TIMELINE, PBR_DEBUG_BOUNDS) keep this
// arrangement, so they measure and check the code the product ships.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "shade_kernels_bal.h"
#include "shade_tile_kernel.h"

namespace pbr {

template <int AMBIENT, bool F0_PLANE, bool APPLY_AO>
hipError_t launch_balanced(const LaunchArgs& a, dim3 grid, hipStream_t stream) {
    if ((a.ps.balanced & kBalKindMask) == 1)
        hipLaunchKernelGGL((shade_tile_kernel<AMBIENT, F0_PLANE, APPLY_AO, false, 1>), grid, dim3(kBlock), 0, stream,
                           a.gb, a.ps, a.lights, a.env, a.frame, a.tile_kept, a.exact_only);
    else
        hipLaunchKernelGGL((shade_tile_kernel<AMBIENT, F0_PLANE, APPLY_AO, false, 2>), grid, dim3(kBlock), 0, stream,
                           a.gb, a.ps, a.lights, a.env, a.frame, a.tile_kept, a.exact_only);
    return hipGetLastError();
}
#define PBR_INSTANTIATE_BAL(A, F, O) template hipError_t launch_balanced<A, F, O>(const LaunchArgs&, dim3, hipStream_t);
PBR_INSTANTIATE_BAL(kAmbientConstant, false, false)
PBR_INSTANTIATE_BAL(kAmbientConstant, false, true)
PBR_INSTANTIATE_BAL(kAmbientConstant, true, false)
PBR_INSTANTIATE_BAL(kAmbientConstant, true, true)
PBR_INSTANTIATE_BAL(kAmbientIblDiffuse, false, false)
PBR_INSTANTIATE_BAL(kAmbientIblDiffuse, false, true)
PBR_INSTANTIATE_BAL(kAmbientIblDiffuse, true, false)
PBR_INSTANTIATE_BAL(kAmbientIblDiffuse, true, true)
#undef PBR_INSTANTIATE_BAL

// PBR_BAL_PROFILE builds: point this unit's kernels at the profile buffer (debug_bal_profile, shade_kernels.hip).
hipError_t debug_bal_profile_publish_bal(unsigned long long* buf) {
#if PBR_BAL_PROFILE
    return hipMemcpyToSymbol(HIP_SYMBOL(g_bal_prof_buf), &buf, sizeof(buf));
#else
    (void)buf;
    return hipErrorNotSupported;
#endif
}

// PBR_WAVE_TIMELINE builds: point this unit's kernels at the timeline buffer (debug_wave_timeline, shade_kernels.hip).
hipError_t debug_wave_timeline_bal(unsigned long long* buf, long long cap) {
#if PBR_WAVE_TIMELINE
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_wave_tl), &buf, sizeof(buf));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_wave_tl_cap), &cap, sizeof(cap));
    return e;
#else
    (void)buf;
    (void)cap;
    return hipErrorNotSupported;
#endif
}

// PBR_DEBUG_BOUNDS builds: point this unit's kernels at the device's bounds-flag buffer (debug_bounds_publish,
// shade_kernels.hip).
hipError_t debug_bounds_publish_bal(uint32_t* buf) {
#if PBR_DEBUG_BOUNDS
    return hipMemcpyToSymbol(HIP_SYMBOL(g_bounds_flags), &buf, sizeof(buf));
#else
    (void)buf;
    return hipErrorNotSupported;
#endif
}

}  // namespace pbr

// This unit's build record (pbr_build_info.h, pbr_build_info): the stamp, flavor and flags it was compiled with and
// every build switch of the kernels as the preprocessor saw it.
#include "pbr_build_info.h"
extern "C" __attribute__((used, visibility("default"))) const char pbr_unit_info_shade_kernels_bal[] =
    PBR_UNIT_INFO("shade_kernels_bal", PBR_KERNEL_SWITCHES);
