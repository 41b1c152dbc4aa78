// shade_common.h -- what every shading kernel shares: the tile, the workgroup's LDS, the register budgets.
//
// One workgroup = one 64x8-pixel screen tile = 256 work-items = 4 wave64s. Work-item t shades the
// horizontal pixel pair (2*(t%32), 2*(t%32)+1) of tile row t/32, so wave w owns tile rows 2w, 2w+1:
// each plane load is one 8-byte load per lane (two full 256-byte row segments per wave) and each
// pair of RGBA stores covers two 1-KiB row segments. The pair is shaded in packed fp32
// (pbr_device_math_x2.h): every light-loop operation except the transcendental seeds and compares
// issues once for both pixels. (The one-pixel kernel, shade_tile1_kernel.h, has 32x8 tiles.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pbr_device_math.h"
#include "pbr_device_math_x2.h"
#include "pbr_balanced.h"
#include "shade_kernels.h"

namespace pbr {
namespace {

constexpr int kTileW = 64;  // pixels; 32 work-items x 2 pixels
constexpr int kTileH = 8;
constexpr int kBlock = 256;
constexpr int kChunk = 256;  // lights staged per LDS pass

// The register budgets (build switches; tools/build_variant.sh varies them).
#ifndef PBR_X2_MIN_WAVES
#define PBR_X2_MIN_WAVES 4  // waves per SIMD the packed kernel is register-allocated for
#endif
#ifndef PBR_LEAN_MIN_WAVES
#define PBR_LEAN_MIN_WAVES 4  // waves per SIMD the culled lean pair kernel is register-allocated for
#endif
#ifndef PBR_LEAN_UNIFORM_MIN_WAVES
#define PBR_LEAN_UNIFORM_MIN_WAVES 5  // ... and the unculled (uniform-loop) faithful or constant-ambient ones
#endif
// Waves per SIMD of shade_lean_kernel<AMBIENT, .., CULL, FAITHFUL>: five for the uniform loops, whose loads wait on HBM
// latency with too few waves to cover it (config 2: DESIGN.md §5d), where 96 VGPRs hold the loop without scratch (the
// faithful ones park albedo and 1 - metallic in LDS across it, lean_wave); four for the culled loops (the culled walk
// and its survivor masks need ~105-116 VGPRs) and for the exact diffuse-IBL loop (20 B/lane of scratch at 96).
template <int AMBIENT, bool CULL, bool FAITHFUL>
constexpr int lean_min_waves() {
    return CULL || (!FAITHFUL && AMBIENT == kAmbientIblDiffuse) ? PBR_LEAN_MIN_WAVES : PBR_LEAN_UNIFORM_MIN_WAVES;
}

// Conservative cull radius: d_fp32 >= d_true * (1 - 4.8e-7) (three roundings in L, three in the
// dot, one in sqrt); a margin of 1e-4 relative covers that and the fp32 box-distance error.
constexpr float kCullRadius = 100.01f;
// PBR_FLAG_FAITHFUL: the most light terms a pixel's sum may have for the mode's error bound.
constexpr int kFaithfulMaxTerms = 64;

struct TileBounds {
    float mn[3], mx[3];
};

__device__ __forceinline__ float wave_min(float v) { return wave_min_dpp(v); }  // pbr_device_math_x2.h
__device__ __forceinline__ float wave_max(float v) { return wave_max_dpp(v); }

struct Lds {
    union {
        float4 light[3 * kChunk];  // the exact re-pass's staged lights
        struct {                   // the balanced point-light pass (pbr_balanced.h)
            BalancedWaveLds bal[kBlock / 64];        // one exchange region per wave
            float bal_light[6 * kBalLdsStride];      // the pass's point lights (stage_balanced_lights)
        };
    };
    int wave_cnt[kBlock / 64];
    float bounds[kBlock / 64][6];
#if PBR_BAL_PROFILE
    unsigned long long prof[kBlock / 64][16];
#endif
    int kept_sum, geo_waves;  // tiled-culling statistics of the block
    int exact_px;             // pixels of the block the exact path redid
};

__device__ __forceinline__ float uniform_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

}  // namespace
}  // namespace pbr

// Every build switch of the shading kernels as the preprocessor saw it, for the build records of the two units that
// compile them (pbr_build_info.h, PBR_UNIT_INFO).
#define PBR_KERNEL_SWITCHES                                                                                   \
    PBR_BI_SWITCH(PBR_X2_MIN_WAVES) ", " PBR_BI_SWITCH(PBR_LEAN_MIN_WAVES) ", "                                 \
    PBR_BI_SWITCH(PBR_LEAN_UNIFORM_MIN_WAVES) ", " PBR_BI_SWITCH(PBR_BAL_PROFILE) ", "                          \
    PBR_BI_SWITCH(PBR_WAVE_TIMELINE) ", " PBR_BI_SWITCH(PBR_DEBUG_BOUNDS) ", "                                  \
    PBR_BI_SWITCH(PBR_POW5_LDS) ", " PBR_BI_SWITCH(PBR_POW5_GLIBC_FROM) ", "                                     \
    PBR_BI_SWITCH(PBR_POW5_FAST3_GLIBC_FROM) ", " PBR_BI_SWITCH(PBR_FAITHFUL_GAMMA_LO) ", "                      \
    PBR_BI_SWITCH(PBR_ATAN2F_KMAX) ", " PBR_BI_SWITCH(PBR_CENSUS)
