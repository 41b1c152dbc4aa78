// material_resolve.h -- the first half of PS on the device (Default.hlsl:50-116): interpolated VertexOut planes and
// the material textures in, the 15 planes of a pbr_gbuffer_soa (plus opacity and coverage) out
// (pbr_resolve_materials, include/pbr/pbr_shade.h). A source of frontend_kernels.hip, which is
// compiled with the canonical fp32 flags: no contraction, correctly rounded / and sqrt.
//
// Layout: a workgroup is 256 threads over a 64 x 8 pixel tile, a lane owns two horizontally adjacent pixels and a
// wave64 covers 64 x 2 pixels (the shading kernels' tile and culling unit), so with 8-byte aligned planes and even
// strides every plane is read and written 8 bytes per lane (VEC), the ids 4 bytes and the coverage 2 bytes; any
// other alignment takes the scalar accesses of the same code. A streaming kernel: ~58 B read and ~65 B written per
// pixel, texel fetches served by L2. No LDS, no barrier, no atomics.
//
// Materials: a wave whose geometry pixels all carry one material id (a ballot against the first geometry lane's
// id) reads that record through a wave-uniform index -- scalar loads, uniform branches on its flags; other waves
// index the table per lane. Both run resolve_pixel, the same fp32 operations in the same order, so the two paths
// are bit-identical.
//
// Textures: every texture is repacked to RGBA8 at upload (pbr_set_materials: a 1-channel texture replicates .r
// into .rgb, a 3-channel one gets alpha 255), all of them in one dword buffer, so a tap is one aligned dword load
// whatever the channel count. A channel decodes as (float)u8 / 255.0f, correctly rounded.
#pragma once

#include "pbr_device_math.h"
#include "frontend_kernels.h"

namespace pbr {

namespace resolve {

// The 14 attribute planes of a pixel in pbr_attributes_soa order.
constexpr int kInPos = 0, kInN = 3, kInT = 6, kInB = 9, kInU = 12, kInV = 13;
struct PixelIn {
    float a[14];
};
struct PixelOut {
    float n[3], alb[3], metal, rough, f0[3], opacity;
    uint32_t cov;
};

__device__ __forceinline__ float unorm8(uint32_t texel, int c) { return (float)((texel >> (8 * c)) & 255u) / 255.0f; }

__device__ __forceinline__ uint32_t tap(const uint32_t* texels, int64_t n_texels, const MaterialTex& t, int x, int y) {
    return texels[PBR_BOUNDS((int64_t)t.offset + (int64_t)(y * t.w + x), n_texels, kBoundsTexel)];
}

// Point-wrap (g_SamPointWrap): the texel that holds (u, v).
__device__ __forceinline__ uint32_t tap_point(const uint32_t* texels, int64_t n_texels, const MaterialTex& t, float u,
                                              float v) {
    const int x = wrap_index(floorf(u * (float)t.w), t.w), y = wrap_index(floorf(v * (float)t.h), t.h);
    return tap(texels, n_texels, t, x, y);
}

// NCH channels of a texture at (u, v): the point tap, or the linear-wrap bilinear of sample_linear_wrap
// (pbr_device_math.h) on the decoded taps.
template <int NCH, bool LINEAR>
__device__ __forceinline__ void sample(const uint32_t* texels, int64_t n_texels, const MaterialTex& t, float u, float v,
                                       float* out) {
    if (!LINEAR) {
        const uint32_t p = tap_point(texels, n_texels, t, u, v);
#pragma unroll
        for (int c = 0; c < NCH; ++c) out[c] = unorm8(p, c);
    } else {
        const float x = u * (float)t.w - 0.5f, y = v * (float)t.h - 0.5f;
        const float x0f = floorf(x), y0f = floorf(y);
        const float fx = x - x0f, fy = y - y0f;
        const int x0 = wrap_index(x0f, t.w), y0 = wrap_index(y0f, t.h);
        const int x1 = x0 + 1 == t.w ? 0 : x0 + 1, y1 = y0 + 1 == t.h ? 0 : y0 + 1;
        const uint32_t t00 = tap(texels, n_texels, t, x0, y0), t10 = tap(texels, n_texels, t, x1, y0),
                       t01 = tap(texels, n_texels, t, x0, y1), t11 = tap(texels, n_texels, t, x1, y1);
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            out[c] = hlerp(hlerp(unorm8(t00, c), unorm8(t10, c), fx), hlerp(unorm8(t01, c), unorm8(t11, c), fx), fy);
    }
}

// Default.hlsl:50-116 for one geometry pixel with material record `m` (a wave-uniform or a per-lane reference).
template <bool LINEAR>
__device__ __forceinline__ void resolve_pixel(const MaterialRec& m, const uint32_t* texels, int64_t n_texels,
                                              const PixelIn& in, PixelOut& o) {
    const uint32_t flags = m.flags;
    // pin.NormalW = normalize(pin.NormalW) (Default.hlsl:50): a zero vector gives NaN, as there
    const float nx = in.a[kInN], ny = in.a[kInN + 1], nz = in.a[kInN + 2];
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    const float nw[3] = {nx / len, ny / len, nz / len};
    if (flags & kMatDiffuseTexture) {
        sample<3, LINEAR>(texels, n_texels, m.tex[0], in.a[kInU], in.a[kInV], o.alb);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.alb[c] = m.diffuse[c];
    }
    if (flags & kMatMetallicTexture)
        sample<1, LINEAR>(texels, n_texels, m.tex[2], in.a[kInU], in.a[kInV], &o.metal);
    else
        o.metal = m.metallic;
    if (flags & kMatSpecularTexture) {
        sample<3, LINEAR>(texels, n_texels, m.tex[1], in.a[kInU], in.a[kInV], o.f0);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.f0[c] = hlerp(m.fresnel[c], o.alb[c], o.metal);  // Default.hlsl:94-95
    }
    if (flags & kMatRoughnessTexture)
        sample<1, LINEAR>(texels, n_texels, m.tex[3], in.a[kInU], in.a[kInV], &o.rough);
    else
        o.rough = m.roughness;
    if (flags & kMatNormalTexture) {  // NormalSampleToWorldSpace (LightingUtil.hlsl:203-214), not renormalised
        float s[3];
        sample<3, LINEAR>(texels, n_texels, m.tex[4], in.a[kInU], in.a[kInV], s);
        const float ntx = 2.0f * s[0] - 1.0f, nty = 2.0f * s[1] - 1.0f, ntz = 2.0f * s[2] - 1.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c)  // mul(normalT, TBN)
            o.n[c] = (ntx * in.a[kInT + c] + nty * in.a[kInB + c]) + ntz * nw[c];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.n[c] = nw[c];
    }
    if (flags & kMatAlphaTest)  // always g_SamPointWrap (Default.hlsl:112)
        o.opacity = unorm8(tap_point(texels, n_texels, m.tex[5], in.a[kInU], in.a[kInV]), 0);
    else
        o.opacity = m.opacity;
    o.cov = 1u;
}

// A background pixel: the host fill's (gbuffer_fill.cpp, fill_reference): NormalW is the sky direction and passes
// through unchanged.
__device__ __forceinline__ void background_pixel(const PixelIn& in, PixelOut& o) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o.n[c] = in.a[kInN + c], o.alb[c] = 0.0f, o.f0[c] = 0.04f;
    o.metal = 0.0f;
    o.rough = 1.0f;
    o.opacity = 1.0f;
    o.cov = 0u;
}

}  // namespace resolve

constexpr int kResolveTileW = 64, kResolveTileH = 8;

template <bool VEC, bool LINEAR>
__global__ __launch_bounds__(256) void resolve_materials_kernel(const ResolveArgs a) {
    using namespace resolve;
    const int x = (int)blockIdx.x * kResolveTileW + (int)(threadIdx.x & 31u) * 2;
    const int y = (int)blockIdx.y * kResolveTileH + (int)(threadIdx.x >> 5);
    const bool in0 = y < a.height && x < a.width, in1 = y < a.height && x + 1 < a.width;
    const bool pair = VEC && in1;  // both pixels through one 8-byte access per plane
    const int64_t ii = (int64_t)y * a.in_stride + x;
    const uint32_t n_mat = (uint32_t)a.n_materials;

    uint32_t id0 = 0xFFFFu, id1 = 0xFFFFu;
    PixelIn p0{}, p1{};
    if (pair) {
        const int64_t i = PBR_BOUNDS_PIXEL(ii, a.width, a.height, a.in_stride, 2, kBoundsGBuffer);
        const uint32_t two = *reinterpret_cast<const uint32_t*>(a.material + i);
        id0 = two & 0xFFFFu;
        id1 = two >> 16;
        float* q0 = p0.a;
        float* q1 = p1.a;
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            const float2 v = *reinterpret_cast<const float2*>(a.attr[k] + i);
            q0[k] = v.x;
            q1[k] = v.y;
        }
    } else {
        if (in0) {
            const int64_t i = PBR_BOUNDS_PIXEL(ii, a.width, a.height, a.in_stride, 1, kBoundsGBuffer);
            id0 = a.material[i];
            float* q0 = p0.a;
#pragma unroll
            for (int k = 0; k < 14; ++k) q0[k] = a.attr[k][i];
        }
        if (in1) {
            const int64_t i = PBR_BOUNDS_PIXEL(ii + 1, a.width, a.height, a.in_stride, 1, kBoundsGBuffer);
            id1 = a.material[i];
            float* q1 = p1.a;
#pragma unroll
            for (int k = 0; k < 14; ++k) q1[k] = a.attr[k][i];
        }
    }
    const bool g0 = in0 && id0 < n_mat, g1 = in1 && id1 < n_mat;

    PixelOut o0, o1;
    background_pixel(p0, o0);
    background_pixel(p1, o1);
    // One material for the whole wave? Every geometry pixel's id against the first geometry lane's.
    const uint32_t key = g0 ? id0 : g1 ? id1 : 0xFFFFFFFFu;
    const uint64_t any = __ballot(key != 0xFFFFFFFFu);
    if (any != 0) {
        const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(any));
        const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
        const bool differs = (g0 && id0 != first) || (g1 && id1 != first);
        if (__ballot(differs) == 0) {
            const MaterialRec& m = a.table[PBR_BOUNDS((int64_t)first, (int64_t)n_mat, kBoundsTexel)];
            if (g0) resolve_pixel<LINEAR>(m, a.texels, a.n_texels, p0, o0);
            if (g1) resolve_pixel<LINEAR>(m, a.texels, a.n_texels, p1, o1);
        } else {
            if (g0)
                resolve_pixel<LINEAR>(a.table[PBR_BOUNDS((int64_t)id0, (int64_t)n_mat, kBoundsTexel)], a.texels,
                                      a.n_texels, p0, o0);
            if (g1)
                resolve_pixel<LINEAR>(a.table[PBR_BOUNDS((int64_t)id1, (int64_t)n_mat, kBoundsTexel)], a.texels,
                                      a.n_texels, p1, o1);
        }
    }

    // pbr_gbuffer_soa order: pos xyz, normal xyz, albedo rgb, metallic, roughness, ao, f0 rgb
    const float v0[15] = {p0.a[0], p0.a[1], p0.a[2], o0.n[0], o0.n[1], o0.n[2], o0.alb[0], o0.alb[1],
                          o0.alb[2], o0.metal, o0.rough, 1.0f, o0.f0[0], o0.f0[1], o0.f0[2]};
    const float v1[15] = {p1.a[0], p1.a[1], p1.a[2], o1.n[0], o1.n[1], o1.n[2], o1.alb[0], o1.alb[1],
                          o1.alb[2], o1.metal, o1.rough, 1.0f, o1.f0[0], o1.f0[1], o1.f0[2]};
    const int64_t oi = (int64_t)y * a.out_stride + x, ci = (int64_t)y * a.cov_stride + x;
    if (pair) {
        const int64_t i = PBR_BOUNDS_PIXEL(oi, a.width, a.height, a.out_stride, 2, kBoundsOutput);
#pragma unroll
        for (int k = 0; k < 15; ++k) *reinterpret_cast<float2*>(a.plane[k] + i) = make_float2(v0[k], v1[k]);
        if (a.opacity) *reinterpret_cast<float2*>(a.opacity + i) = make_float2(o0.opacity, o1.opacity);
        if (a.coverage)
            *reinterpret_cast<uint16_t*>(a.coverage +
                                         PBR_BOUNDS_PIXEL(ci, a.width, a.height, a.cov_stride, 2, kBoundsCoverage)) =
                (uint16_t)(o0.cov | (o1.cov << 8));
    } else {
        if (in0) {
            const int64_t i = PBR_BOUNDS_PIXEL(oi, a.width, a.height, a.out_stride, 1, kBoundsOutput);
#pragma unroll
            for (int k = 0; k < 15; ++k) a.plane[k][i] = v0[k];
            if (a.opacity) a.opacity[i] = o0.opacity;
            if (a.coverage)
                a.coverage[PBR_BOUNDS_PIXEL(ci, a.width, a.height, a.cov_stride, 1, kBoundsCoverage)] = (uint8_t)o0.cov;
        }
        if (in1) {
            const int64_t i = PBR_BOUNDS_PIXEL(oi + 1, a.width, a.height, a.out_stride, 1, kBoundsOutput);
#pragma unroll
            for (int k = 0; k < 15; ++k) a.plane[k][i] = v1[k];
            if (a.opacity) a.opacity[i] = o1.opacity;
            if (a.coverage)
                a.coverage[PBR_BOUNDS_PIXEL(ci + 1, a.width, a.height, a.cov_stride, 1, kBoundsCoverage)] =
                    (uint8_t)o1.cov;
        }
    }
}

hipError_t launch_resolve_materials(const ResolveArgs& a, hipStream_t stream) {
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid((a.width + kResolveTileW - 1) / kResolveTileW, (a.height + kResolveTileH - 1) / kResolveTileH);
    if (a.vec) {
        if (a.linear)
            hipLaunchKernelGGL((resolve_materials_kernel<true, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((resolve_materials_kernel<true, false>), grid, dim3(256), 0, stream, a);
    } else {
        if (a.linear)
            hipLaunchKernelGGL((resolve_materials_kernel<false, true>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((resolve_materials_kernel<false, false>), grid, dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace pbr
