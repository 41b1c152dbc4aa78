// shade_kernels_bal.h -- what shade_kernels_bal.hip (the wave-balanced kernels' unit) defines for shade_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "shade_kernels.h"

namespace pbr {

// Launches the balanced variant (a.ps.balanced 1 or 2) of shade_tile_kernel over `grid`.
template <int AMBIENT, bool F0_PLANE, bool APPLY_AO>
hipError_t launch_balanced(const LaunchArgs& a, dim3 grid, hipStream_t stream);

// That unit's copies of the development builds' device pointers (g_bal_prof_buf, g_wave_tl, g_bounds_flags): each
// publisher of shade_kernels.hip sets its own unit's copy and chains to the one here.
hipError_t debug_bal_profile_publish_bal(unsigned long long* buf);
hipError_t debug_wave_timeline_bal(unsigned long long* buf, long long cap);
hipError_t debug_bounds_publish_bal(uint32_t* buf);

}  // namespace pbr
