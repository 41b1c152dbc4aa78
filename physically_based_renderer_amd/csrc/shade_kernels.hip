// shade_kernels.hip -- the shading kernels' main unit: the launch and dispatch ladder of pbr_shade, and every shading
// kernel it launches except the wave-balanced ones. The kernels are in headers, one per kernel family:
//   shade_tile_kernel.h   the pair kernel that carries every path (sky pass, EXACT_ONLY; BAL 0 here);
//   shade_lean_kernel.h   the lean pair kernel (uniform and culled loops without a sky pass);
//   shade_tile1_kernel.h  one pixel per work-item;
// over shade_common.h (tile, LDS), shade_light_loops.h, shade_pixel.h (load, finish, store) and the development
// instrumentation of shade_wave_timeline.h. The balanced kernels (shade_tile_kernel BAL 1, 2) are compiled in
// shade_kernels_bal.hip, which says why; shade_kernels_bal.h is what that unit defines for this one.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "shade_kernels.h"
#include "shade_kernels_bal.h"
#include "shade_lean_kernel.h"
#include "shade_tile1_kernel.h"
#include "shade_tile_kernel.h"

namespace pbr {

// Development builds with PBR_BAL_PROFILE: read (and optionally clear) the kernels' clock sums (pbr_balanced.h; both
// units' kernels add into disjoint slots of the one buffer).
hipError_t debug_bal_profile(unsigned long long* out8, bool reset) {
#if PBR_BAL_PROFILE
    constexpr size_t kWaves = 1 << 18, kBytes = kWaves * 16 * sizeof(unsigned long long);
    static unsigned long long* buf = nullptr;
    hipError_t e = hipSuccess;
    if (!buf) {
        e = hipMalloc(&buf, kBytes);
        if (e == hipSuccess) e = hipMemset(buf, 0, kBytes);
        if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_bal_prof_buf), &buf, sizeof(buf));
        if (e == hipSuccess) e = debug_bal_profile_publish_bal(buf);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    std::vector<unsigned long long> h(kWaves * 16);
    if (e == hipSuccess) e = hipMemcpy(h.data(), buf, kBytes, hipMemcpyDeviceToHost);
    for (int i = 0; i < 16; ++i) out8[i] = 0;
    for (size_t w = 0; w < kWaves; ++w)
        for (int i = 0; i < 16; ++i) out8[i] += h[w * 16 + i];
    if (e == hipSuccess && reset) e = hipMemset(buf, 0, kBytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
#else
    (void)out8;
    (void)reset;
    return hipErrorNotSupported;
#endif
}

// Development builds with PBR_WAVE_TIMELINE: point both units' kernels at a device buffer of cap * kTlWords words
// (nullptr: off).
hipError_t debug_wave_timeline(unsigned long long* buf, long long cap) {
#if PBR_WAVE_TIMELINE
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_wave_tl), &buf, sizeof(buf));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_wave_tl_cap), &cap, sizeof(cap));
    if (e == hipSuccess) e = debug_wave_timeline_bal(buf, cap);
    return e;
#else
    (void)buf;
    (void)cap;
    return hipErrorNotSupported;
#endif
}

// PBR_DEBUG_BOUNDS builds: point both units' kernels at the device's bounds-flag buffer
// (2 * kBoundsClasses words, pbr_debug_bounds.h; one process-wide buffer per device, current device).
hipError_t debug_bounds_publish(uint32_t* buf) {
#if PBR_DEBUG_BOUNDS
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_bounds_flags), &buf, sizeof(buf));
    if (e == hipSuccess) e = debug_bounds_publish_bal(buf);
    return e;
#else
    (void)buf;
    return hipErrorNotSupported;
#endif
}

__global__ void decode_unorm16_kernel(const uint16_t* __restrict__ src, float4* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const ushort4 t = reinterpret_cast<const ushort4*>(src)[i];
        // R16G16B16A16_UNORM decode (WICTextureLoader.cpp:312-367): value / 65535
        dst[i] = make_float4((float)t.x / 65535.0f, (float)t.y / 65535.0f, (float)t.z / 65535.0f, (float)t.w / 65535.0f);
    }
}

template <int AMBIENT, bool F0_PLANE, bool APPLY_AO, bool CULL>
static hipError_t launch_variant(const LaunchArgs& a, hipStream_t stream) {
    if (a.pixels_per_thread == 2) {
        dim3 grid((a.gb.width + kTileW - 1) / kTileW, (a.gb.height + kTileH - 1) / kTileH);
        if (!CULL && a.ps.balanced != 0)
            return launch_balanced<AMBIENT, F0_PLANE, APPLY_AO>(a, grid, stream);
        if (a.lean) {  // uniform loops, no sky pass (shade_lean_kernel): one wave per workgroup
            const dim3 wgrid(grid.x, grid.y * (kBlock / 64));
            if (a.ps.faithful)
                hipLaunchKernelGGL((shade_lean_kernel<AMBIENT, F0_PLANE, APPLY_AO, CULL, true>), wgrid, dim3(64), 0,
                                   stream, a.gb, a.ps, a.lights, a.env, a.frame, a.tile_kept);
            else
                hipLaunchKernelGGL((shade_lean_kernel<AMBIENT, F0_PLANE, APPLY_AO, CULL, false>), wgrid, dim3(64), 0,
                                   stream, a.gb, a.ps, a.lights, a.env, a.frame, a.tile_kept);
        } else
            hipLaunchKernelGGL((shade_tile_kernel<AMBIENT, F0_PLANE, APPLY_AO, CULL>), grid, dim3(kBlock), 0, stream,
                               a.gb, a.ps, a.lights, a.env, a.frame, a.tile_kept, a.exact_only);
    } else {
        dim3 grid((a.gb.width + kTileW1 - 1) / kTileW1, (a.gb.height + kTileH - 1) / kTileH);
        hipLaunchKernelGGL((shade_tile1_kernel<AMBIENT, F0_PLANE, APPLY_AO, CULL>), grid, dim3(kBlock), 0, stream,
                           a.gb, a.ps, a.lights, a.env, a.frame, a.tile_kept, a.exact_only);
    }
    return hipGetLastError();
}

template <int AMBIENT, bool F0_PLANE, bool APPLY_AO>
static hipError_t dispatch_cull(const LaunchArgs& a, hipStream_t s) {
    return a.cull ? launch_variant<AMBIENT, F0_PLANE, APPLY_AO, true>(a, s)
                  : launch_variant<AMBIENT, F0_PLANE, APPLY_AO, false>(a, s);
}
template <int AMBIENT, bool F0_PLANE>
static hipError_t dispatch_ao(const LaunchArgs& a, hipStream_t s) {
    return a.apply_ao ? dispatch_cull<AMBIENT, F0_PLANE, true>(a, s) : dispatch_cull<AMBIENT, F0_PLANE, false>(a, s);
}
template <int AMBIENT>
static hipError_t dispatch_f0(const LaunchArgs& a, hipStream_t s) {
    return a.f0_plane ? dispatch_ao<AMBIENT, true>(a, s) : dispatch_ao<AMBIENT, false>(a, s);
}

hipError_t launch_shade(const LaunchArgs& a, hipStream_t stream) {
    if (a.gb.width <= 0 || a.gb.height <= 0) return hipSuccess;
    return a.ambient_mode == kAmbientIblDiffuse ? dispatch_f0<kAmbientIblDiffuse>(a, stream)
                                                : dispatch_f0<kAmbientConstant>(a, stream);
}

std::string launched_kernel(const LaunchArgs& a) {
    if (a.gb.width <= 0 || a.gb.height <= 0) return "";
    auto b = [](bool v) { return v ? std::string("true") : std::string("false"); };
    const std::string t = std::to_string(a.ambient_mode == kAmbientIblDiffuse ? 1 : 0) + ", " + b(a.f0_plane) + ", " +
                          b(a.apply_ao) + ", " + b(a.cull);
    if (a.pixels_per_thread != 2) return "shade_tile1_kernel<" + t + ">";
    if (!a.cull && a.ps.balanced != 0) return "shade_tile_kernel<" + t + ", " + std::to_string(a.ps.balanced & kBalKindMask) + ">";
    if (a.lean) return "shade_lean_kernel<" + t + ", " + b(a.ps.faithful != 0) + ">";
    return "shade_tile_kernel<" + t + ", 0>";
}

int64_t shade_tile_count(int width, int height, int pixels_per_thread) {
    const int tw = pixels_per_thread == 2 ? kTileW : kTileW1;
    return (int64_t)((width + tw - 1) / tw) * ((height + kTileH - 1) / kTileH);
}

int shade_stat_slots_per_tile(int pixels_per_thread) { return pixels_per_thread == 2 ? kBlock / 64 : 1; }

hipError_t launch_decode_unorm16(const uint16_t* src, float4* dst, int n_texels, hipStream_t stream) {
    if (n_texels <= 0) return hipSuccess;
    hipLaunchKernelGGL(decode_unorm16_kernel, dim3((n_texels + 255) / 256), dim3(256), 0, stream, src, dst, n_texels);
    return hipGetLastError();
}

}  // namespace pbr

// This unit's build record (pbr_build_info.h, pbr_build_info): the stamp, flavor and flags it was compiled with and
// every build switch of the kernels as the preprocessor saw it.
#include "pbr_build_info.h"
extern "C" __attribute__((used, visibility("default"))) const char pbr_unit_info_shade_kernels[] =
    PBR_UNIT_INFO("shade_kernels", PBR_KERNEL_SWITCHES);
