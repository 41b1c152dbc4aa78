// msaa_resolve.h -- the output merger's multisample resolve on the device (pbr_msaa_resolve, include/pbr/pbr_shade.h;
// DESIGN.md §12 step 7b): the four samples of a pixel, each the shaded colour of the slot that owns it, averaged into
// one pixel. A source of frontend_kernels.hip, compiled with the canonical fp32 flags (no contraction).
//
// Per pixel, with o the owner byte, k_s = (o >> 2s) & 3 and c_s the pixel of slot frame k_s (0 in every channel when
// k_s >= n_slots; that frame's pointer is then never read), per channel, alpha included:
//   RGBA32F:     out = ((c_0 + c_1) + (c_2 + c_3)) * 0.25f, each operation rounded once. Pairwise, so that four equal
//                inputs give themselves bit for bit.
//   RGBA8_UNORM: a sample of a UNORM8 multisampled target holds unorm8(clamp(c_s)) (clamp: pbr_blend_layer's rule,
//                NaN -> 0); d_s = (float)byte / 255.0f, the same expression, unorm8 (pbr_unorm.h) of the result.
// One pixel per lane, 256 threads over a 64 x 4 tile. A slot frame is loaded only where some sample of the pixel is
// owned by it: where one fragment owns the pixel -- almost everywhere -- that is one load. With VEC one 16-byte access
// per pixel and frame, else 4-byte accesses.
#pragma once

#include "blend_layer.h"
#include "frontend_kernels.h"
#include "pbr_debug_bounds.h"
#include "pbr_unorm.h"

namespace pbr {

namespace msaa {

__device__ __forceinline__ float resolve_channel(float c0, float c1, float c2, float c3) {
    return ((c0 + c1) + (c2 + c3)) * 0.25f;
}
__device__ __forceinline__ float pick(int k, float f0, float f1, float f2, float f3) {
    return k == 0 ? f0 : (k == 1 ? f1 : (k == 2 ? f2 : f3));
}
// What a UNORM8 sample gives back: the stored byte, decoded.
__device__ __forceinline__ float unorm8_sample(float c) {
    return (float)unorm8(blend::saturate_input(c)) / 255.0f;
}

}  // namespace msaa

template <bool VEC, int FORMAT>
__global__ __launch_bounds__(256) void msaa_resolve_kernel(const MsaaResolveArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63u);
    const int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const uint32_t o = a.owner[PBR_BOUNDS_PIXEL((int64_t)y * a.owner_stride + x, a.width, a.height, a.owner_stride, 1,
                                                kBoundsRaster)];
    const int k0 = (int)(o & 3u), k1 = (int)((o >> 2) & 3u), k2 = (int)((o >> 4) & 3u), k3 = (int)(o >> 6);
    const int64_t si = PBR_BOUNDS_PIXEL((int64_t)y * a.slot_stride + x, a.width, a.height, a.slot_stride, 1,
                                        kBoundsRaster);
    float f[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool used = k < a.n_slots && (k0 == k || k1 == k || k2 == k || k3 == k);
#pragma unroll
        for (int c = 0; c < 4; ++c) f[k][c] = 0.0f;
        if (used) {
            const float* p = a.slots[k] + 4 * si;
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(p);
                f[k][0] = t.x, f[k][1] = t.y, f[k][2] = t.z, f[k][3] = t.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) f[k][c] = p[c];
            }
        }
    }
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // any owner byte is taken as it is, also one the fragments stage never writes (sample 0 not in slot 0)
        float c0 = msaa::pick(k0, f[0][c], f[1][c], f[2][c], f[3][c]);
        float c1 = msaa::pick(k1, f[0][c], f[1][c], f[2][c], f[3][c]);
        float c2 = msaa::pick(k2, f[0][c], f[1][c], f[2][c], f[3][c]);
        float c3 = msaa::pick(k3, f[0][c], f[1][c], f[2][c], f[3][c]);
        if constexpr (FORMAT == kBlendRgba8) {
            c0 = msaa::unorm8_sample(c0), c1 = msaa::unorm8_sample(c1);
            c2 = msaa::unorm8_sample(c2), c3 = msaa::unorm8_sample(c3);
        }
        r[c] = msaa::resolve_channel(c0, c1, c2, c3);
    }
    const int64_t oi = PBR_BOUNDS_PIXEL((int64_t)y * a.out_stride + x, a.width, a.height, a.out_stride, 1, kBoundsOutput);
    if constexpr (FORMAT == kBlendRgba8) {
        static_cast<uint32_t*>(a.out)[oi] = unorm8(r[0]) | (unorm8(r[1]) << 8) | (unorm8(r[2]) << 16) | (unorm8(r[3]) << 24);
    } else {
        float* out = static_cast<float*>(a.out) + 4 * oi;
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(out) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) out[c] = r[c];
        }
    }
}

hipError_t launch_msaa_resolve(const MsaaResolveArgs& a, hipStream_t stream) {
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid((a.width + 63) / 64, (a.height + 3) / 4);
    if (a.format == kBlendRgba8) {
        if (a.vec)
            hipLaunchKernelGGL((msaa_resolve_kernel<true, kBlendRgba8>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((msaa_resolve_kernel<false, kBlendRgba8>), grid, dim3(256), 0, stream, a);
    } else if (a.vec) {
        hipLaunchKernelGGL((msaa_resolve_kernel<true, kBlendRgba32f>), grid, dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL((msaa_resolve_kernel<false, kBlendRgba32f>), grid, dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace pbr
