// blend_layer.h -- the output-merger blend of the reference's transparent PSO (PBRApp.cpp:831-842) on the device
// (pbr_blend_layer, include/pbr/pbr_shade.h): colour SRC_ALPHA / INV_SRC_ALPHA with op ADD, alpha
// ONE / ZERO with op ADD, of a shaded layer over a frame. A source of frontend_kernels.hip, compiled with the canonical
// fp32 flags (no contraction).
//
// Per pixel the layer covers (coverage != 0), with a the alpha plane's value and s the source colour:
//   RGBA32F:     out.c = (s.c * a) + (d.c * (1.0f - a)), out.a = a.
//   RGBA8_UNORM: d.c = (float)byte / 255.0f; s.c and a are first clamped to [0, 1] with NaN -> 0 (the fixed-point
//                render-target rule); the same expression; the four results go through unorm8 (pbr_unorm.h).
// A pixel with coverage 0 is neither read nor written in the destination. The layout is the front end's: 256 threads
// over a 64 x 8 tile, a pixel pair per lane; with VEC one 16-byte access per RGBA32F pixel, else 4-byte accesses.
#pragma once

#include "frontend_kernels.h"
#include "pbr_debug_bounds.h"
#include "pbr_unorm.h"

namespace pbr {

namespace blend {

// The fixed-point render-target rule for a blend input: NaN -> 0, clamp to [0, 1].
__device__ __forceinline__ float saturate_input(float v) {
    if (!(v == v)) return 0.0f;
    v = v > 1.0f ? 1.0f : v;
    return v < 0.0f ? 0.0f : v;
}

__device__ __forceinline__ float blend_channel(float s, float d, float a) { return (s * a) + (d * (1.0f - a)); }

template <bool VEC, int FORMAT>
__device__ __forceinline__ void blend_pixel(const BlendArgs& a, int x, int y) {
    const int64_t ci = PBR_BOUNDS_PIXEL((int64_t)y * a.cov_stride + x, a.width, a.height, a.cov_stride, 1,
                                        kBoundsCoverage);
    if (a.coverage[ci] == 0) return;
    const int64_t ai = PBR_BOUNDS_PIXEL((int64_t)y * a.alpha_stride + x, a.width, a.height, a.alpha_stride, 1,
                                        kBoundsGBuffer);
    const int64_t si = PBR_BOUNDS_PIXEL((int64_t)y * a.src_stride + x, a.width, a.height, a.src_stride, 1,
                                        kBoundsGBuffer);
    const int64_t oi = PBR_BOUNDS_PIXEL((int64_t)y * a.out_stride + x, a.width, a.height, a.out_stride, 1,
                                        kBoundsOutput);
    float al = a.alpha[ai];
    float s[3];
    if constexpr (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(a.src + 4 * si);
        s[0] = t.x, s[1] = t.y, s[2] = t.z;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = a.src[4 * si + c];
    }
    if constexpr (FORMAT == kBlendRgba8) {
        uint32_t* out = static_cast<uint32_t*>(a.out) + oi;
        const uint32_t d = *out;
        al = saturate_input(al);
        uint32_t r = unorm8(al) << 24;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float dc = (float)((d >> (8 * c)) & 255u) / 255.0f;
            r |= unorm8(blend_channel(saturate_input(s[c]), dc, al)) << (8 * c);
        }
        *out = r;
    } else {
        float* out = static_cast<float*>(a.out) + 4 * oi;
        if constexpr (VEC) {
            const float4 d = *reinterpret_cast<const float4*>(out);
            *reinterpret_cast<float4*>(out) = make_float4(blend_channel(s[0], d.x, al), blend_channel(s[1], d.y, al),
                                                          blend_channel(s[2], d.z, al), al);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = blend_channel(s[c], out[c], al);
            out[3] = al;
        }
    }
}

}  // namespace blend

template <bool VEC, int FORMAT>
__global__ __launch_bounds__(256) void blend_layer_kernel(const BlendArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 31u) * 2;
    const int y = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);
    if (y >= a.height) return;
    if (x < a.width) blend::blend_pixel<VEC, FORMAT>(a, x, y);
    if (x + 1 < a.width) blend::blend_pixel<VEC, FORMAT>(a, x + 1, y);
}

hipError_t launch_blend_layer(const BlendArgs& a, hipStream_t stream) {
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid((a.width + 63) / 64, (a.height + 7) / 8);
    if (a.format == kBlendRgba8) {
        if (a.vec)
            hipLaunchKernelGGL((blend_layer_kernel<true, kBlendRgba8>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((blend_layer_kernel<false, kBlendRgba8>), grid, dim3(256), 0, stream, a);
    } else if (a.vec) {
        hipLaunchKernelGGL((blend_layer_kernel<true, kBlendRgba32f>), grid, dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL((blend_layer_kernel<false, kBlendRgba32f>), grid, dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace pbr
