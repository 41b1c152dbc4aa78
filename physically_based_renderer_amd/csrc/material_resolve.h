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
//
// Mip chains and the trilinear filter (pbr_generate_mips, pbr_resolve_materials_mip; the reference samples its maps over
// texture->Resource->GetDesc().MipLevels levels, PBRApp.cpp:701, :1171-1178, Default.hlsl:80-105): the chains are built
// by generate_mip_level_kernel, one launch per level; resolve_materials_mip_kernel is the same tile, pixel pair per
// lane and record paths as resolve_materials_kernel, with the level of detail of each sampled texture taken from the
// differences of u and v inside the 2 x 2 pixel quad a wave holds: across the lane's own pair, and across lanes L and
// L ^ 32 (the rows y and y ^ 1) through one half-wave swap per value.
//
// The anisotropic filter (pbr_resolve_materials_aniso; the reference's sampler is D3D12_FILTER_ANISOTROPIC with
// maxAnisotropy 8, PBRApp.cpp:1171-1178): resolve_materials_aniso_kernel is the trilinear kernel around another sampler:
// the same footprints give a tap count per texture, the level comes from the shorter footprint axis, and the taps along
// the longer one are fetched in a loop.
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

// The point or the linear filter on level 0: the sampler of resolve_materials_kernel.
template <bool LINEAR>
struct LevelZero {
    // NCH channels of the material's map `slot` (its tex[] index), whose level 0 is `t` in `texels`.
    template <int NCH>
    __device__ __forceinline__ void fetch(const uint32_t* texels, int64_t n_texels, const MaterialTex& t, int slot,
                                          float u, float v, float* out) const {
        sample<NCH, LINEAR>(texels, n_texels, t, u, v, out);
    }
};

// The screen-space differences of (u, v) at a pixel: right minus left and bottom minus top inside its
// 2 x 2 quad, +0 where the partner is outside the frame or has another material.
struct Footprint {
    float dudx, dvdx, dudy, dvdy;
};

// The trilinear filter over a material's mip chains: the sampler of resolve_materials_mip_kernel. `slots`: the five
// MipSlot of the pixel's material.
struct Trilinear {
    const ResolveMipArgs& a;
    const MipSlot* slots;
    Footprint d;
    template <int NCH>
    __device__ __forceinline__ void fetch(const uint32_t*, int64_t, const MaterialTex& t, int slot, float u, float v,
                                          float* out) const {
        const MipSlot chain = slots[slot];
        const int last = chain.levels - 1;
        const float ax = d.dudx * (float)t.w, ay = d.dvdx * (float)t.h;
        const float bx = d.dudy * (float)t.w, by = d.dvdy * (float)t.h;
        const float rx = ax * ax + ay * ay, ry = bx * bx + by * by;
        const float r2 = ry > rx ? ry : rx;
        float base = 0.0f;
        if (r2 > 1.0f) {  // false for NaN; the piecewise-linear log2: exponent plus mantissa fraction
            const uint32_t b = __float_as_uint(r2);
            const float l2 = (float)((int)(b >> 23) - 127) + (float)(b & 0x7FFFFFu) * 0x1p-23f;
            base = 0.5f * l2;
        }
        float lod = base + a.lod_bias;
        if (lod < 0.0f) lod = 0.0f;
        if (lod > (float)last) lod = (float)last;
        const int l0 = (int)floorf(lod);
        const float f = lod - (float)l0;
        level<NCH>(t, chain, l0, u, v, out);
        if (f != 0.0f) {  // f == 0: c0 + 0 * (c1 - c0) has c0's bits
            const int l1 = l0 + 1 < last ? l0 + 1 : last;
            float c1[NCH];
            level<NCH>(t, chain, l1, u, v, c1);
#pragma unroll
            for (int c = 0; c < NCH; ++c) out[c] = hlerp(out[c], c1[c], f);
        }
    }
    // The linear-wrap bilinear of level l: level 0 in the upload's buffer, the others in the chains'.
    template <int NCH>
    __device__ __forceinline__ void level(const MaterialTex& t, const MipSlot& chain, int l, float u, float v,
                                          float* out) const {
        if (l == 0) {
            sample<NCH, true>(a.r.texels, a.r.n_texels, t, u, v, out);
        } else {
            const MaterialTex tl = a.levels[PBR_BOUNDS((int64_t)chain.first + (l - 1), a.n_levels, kBoundsTexel)];
            sample<NCH, true>(a.mip_texels, a.n_mip_texels, tl, u, v, out);
        }
    }
};

// Default.hlsl:50-116 for one geometry pixel with material record `m` (a wave-uniform or a per-lane reference); `s`
// samples its five maps.
template <class Sampler>
__device__ __forceinline__ void resolve_pixel(const MaterialRec& m, const uint32_t* texels, int64_t n_texels,
                                              const PixelIn& in, PixelOut& o, const Sampler& s) {
    const uint32_t flags = m.flags;
    // pin.NormalW = normalize(pin.NormalW) (Default.hlsl:50): a zero vector gives NaN, as there
    const float nx = in.a[kInN], ny = in.a[kInN + 1], nz = in.a[kInN + 2];
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    const float nw[3] = {nx / len, ny / len, nz / len};
    if (flags & kMatDiffuseTexture) {
        s.template fetch<3>(texels, n_texels, m.tex[0], 0, in.a[kInU], in.a[kInV], o.alb);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.alb[c] = m.diffuse[c];
    }
    if (flags & kMatMetallicTexture)
        s.template fetch<1>(texels, n_texels, m.tex[2], 2, in.a[kInU], in.a[kInV], &o.metal);
    else
        o.metal = m.metallic;
    if (flags & kMatSpecularTexture) {
        s.template fetch<3>(texels, n_texels, m.tex[1], 1, in.a[kInU], in.a[kInV], o.f0);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.f0[c] = hlerp(m.fresnel[c], o.alb[c], o.metal);  // Default.hlsl:94-95
    }
    if (flags & kMatRoughnessTexture)
        s.template fetch<1>(texels, n_texels, m.tex[3], 3, in.a[kInU], in.a[kInV], &o.rough);
    else
        o.rough = m.roughness;
    if (flags & kMatNormalTexture) {  // NormalSampleToWorldSpace (LightingUtil.hlsl:203-214), not renormalised
        float smp[3];
        s.template fetch<3>(texels, n_texels, m.tex[4], 4, in.a[kInU], in.a[kInV], smp);
        const float ntx = 2.0f * smp[0] - 1.0f, nty = 2.0f * smp[1] - 1.0f, ntz = 2.0f * smp[2] - 1.0f;
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

// A value of the wave's two rows: .x from the even row (lanes 0-31), .y from the odd one (lanes 32-63), in every lane
// of both. One v_permlane32_swap; every lane of the wave must call it.
__device__ __forceinline__ uint2 quad_rows(uint32_t v) {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return make_uint2(r[0], r[1]);
}
__device__ __forceinline__ float rows_difference(float v) {  // bottom minus top
    const uint2 r = quad_rows(__float_as_uint(v));
    return __uint_as_float(r.y) - __uint_as_float(r.x);
}

// The footprints of both pixels of a lane. Every lane of the wave must call it. A partner outside the frame carries id
// 0xFFFF, which no geometry pixel has: comparing ids is the whole validity test of a geometry pixel's partner (a
// background pixel's footprint is never read).
__device__ __forceinline__ void quad_footprints(const PixelIn& p0, const PixelIn& p1, uint32_t id0, uint32_t id1,
                                                Footprint d[2]) {
    const float dudy0 = rows_difference(p0.a[kInU]), dvdy0 = rows_difference(p0.a[kInV]);
    const float dudy1 = rows_difference(p1.a[kInU]), dvdy1 = rows_difference(p1.a[kInV]);
    const uint2 ids = quad_rows(id0 | (id1 << 16));
    const bool h = id0 == id1, v0 = (ids.x & 0xFFFFu) == (ids.y & 0xFFFFu), v1 = (ids.x >> 16) == (ids.y >> 16);
    const float dudx = h ? p1.a[kInU] - p0.a[kInU] : 0.0f, dvdx = h ? p1.a[kInV] - p0.a[kInV] : 0.0f;
    d[0] = Footprint{dudx, dvdx, v0 ? dudy0 : 0.0f, v0 ? dvdy0 : 0.0f};
    d[1] = Footprint{dudx, dvdx, v1 ? dudy1 : 0.0f, v1 ? dvdy1 : 0.0f};
}

// The sampler of a pixel with material `id` (wave-uniform or per lane) and footprint `d`.
__device__ __forceinline__ Trilinear trilinear(const ResolveMipArgs& a, uint32_t id, const Footprint& d) {
    return {a, a.slots + PBR_BOUNDS((int64_t)id * 5, (int64_t)a.r.n_materials * 5, kBoundsTexel), d};
}

// The anisotropic filter over a material's mip chains ("Anisotropic filter"): the sampler of
// resolve_materials_aniso_kernel. The level comes from the shorter of the two screen-axis footprints, N <= max_aniso
// bilinear taps are spread along the longer one, averaged per level, and the two levels are mixed once. The level loop
// and the tap loop are real loops with per-lane trip counts (1 or 2, and 1 .. 16): they run inside divergent code and
// hold no cross-lane operation; a fetch inlines one bilinear, not one per tap and level.
struct Anisotropic {
    const ResolveAnisoArgs& a;
    const MipSlot* slots;
    Footprint d;
    template <int NCH>
    __device__ __forceinline__ void fetch(const uint32_t*, int64_t, const MaterialTex& t, int slot, float u, float v,
                                          float* out) const {
        const ResolveMipArgs& ma = a.m;
        const MipSlot chain = slots[slot];
        const int last = chain.levels - 1;
        const float ax = d.dudx * (float)t.w, ay = d.dvdx * (float)t.h;
        const float bx = d.dudy * (float)t.w, by = d.dvdy * (float)t.h;
        const float rx = ax * ax + ay * ay, ry = bx * bx + by * by;
        const bool ymajor = ry > rx;  // false for NaN
        const float pmax2 = ymajor ? ry : rx, pmin2 = ymajor ? rx : ry;
        const float du = ymajor ? d.dudy : d.dudx, dv = ymajor ? d.dvdy : d.dvdx;  // UV units
        // The smallest n with pmax2 <= n^2 pmin2, at most max_aniso: NaN gives 1, a zero minor axis under a non-zero
        // major one gives max_aniso. A compare and a select per step; the trip count is wave-uniform (a kernel
        // argument), so max_aniso = 1 pays for no step.
        int n = 1;
#pragma unroll 1
        for (int k = 1; k < a.max_aniso; ++k)
            if (pmax2 > (float)(k * k) * pmin2) n = k + 1;
        const bool many = n > 1;  // a lane with one tap takes none of the divisions below
        const float fn = (float)n;
        float r2 = pmax2;
        if (many) r2 = pmax2 / (float)(n * n);
        float base = 0.0f;
        if (r2 > 1.0f) {  // false for NaN; the piecewise-linear log2: exponent plus mantissa fraction
            const uint32_t b = __float_as_uint(r2);
            const float l2 = (float)((int)(b >> 23) - 127) + (float)(b & 0x7FFFFFu) * 0x1p-23f;
            base = 0.5f * l2;
        }
        float lod = base + ma.lod_bias;
        if (lod < 0.0f) lod = 0.0f;
        if (lod > (float)last) lod = (float)last;
        const int l0 = (int)floorf(lod);
        const float f = lod - (float)l0;
        const int l1 = l0 + 1 < last ? l0 + 1 : last;
        const int n_pass = f != 0.0f ? 2 : 1;  // f == 0: c0 + 0 * (c1 - c0) has c0's bits
        const float two_n = (float)(2 * n);
#pragma unroll
        for (int c = 0; c < NCH; ++c) out[c] = 0.0f;
#pragma unroll 1
        for (int pass = 0; pass < n_pass; ++pass) {
            // The level's texels and size, once per level: level 0 in the upload's buffer, the others in the chains'.
            const int l = pass == 0 ? l0 : l1;
            const uint32_t* texels = ma.r.texels;
            int64_t n_texels = ma.r.n_texels;
            MaterialTex tl = t;
            if (l != 0) {
                tl = ma.levels[PBR_BOUNDS((int64_t)chain.first + (l - 1), ma.n_levels, kBoundsTexel)];
                texels = ma.mip_texels;
                n_texels = ma.n_mip_texels;
            }
            float s[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) s[c] = 0.0f;
#pragma unroll 1
            for (int i = 0; i < n; ++i) {
                // Centred on (u, v), evenly spaced, spanning (N - 1) / N of the major axis; N == 1: (u, v) itself.
                float ui = u, vi = v;
                if (many) {
                    const float ti = (float)(2 * i + 1 - n) / two_n;
                    ui = u + ti * du;
                    vi = v + ti * dv;
                }
                float b[NCH];
                sample<NCH, true>(texels, n_texels, tl, ui, vi, b);
#pragma unroll
                for (int c = 0; c < NCH; ++c) s[c] = i == 0 ? b[c] : s[c] + b[c];
            }
            if (many) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) s[c] = s[c] / fn;
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) out[c] = pass == 0 ? s[c] : hlerp(out[c], s[c], f);
        }
    }
};

// The sampler of a pixel with material `id` (wave-uniform or per lane) and footprint `d`.
__device__ __forceinline__ Anisotropic anisotropic(const ResolveAnisoArgs& a, uint32_t id, const Footprint& d) {
    return {a, a.m.slots + PBR_BOUNDS((int64_t)id * 5, (int64_t)a.m.r.n_materials * 5, kBoundsTexel), d};
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

    const LevelZero<LINEAR> level0;
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
            if (g0) resolve_pixel(m, a.texels, a.n_texels, p0, o0, level0);
            if (g1) resolve_pixel(m, a.texels, a.n_texels, p1, o1, level0);
        } else {
            if (g0)
                resolve_pixel(a.table[PBR_BOUNDS((int64_t)id0, (int64_t)n_mat, kBoundsTexel)], a.texels, a.n_texels,
                              p0, o0, level0);
            if (g1)
                resolve_pixel(a.table[PBR_BOUNDS((int64_t)id1, (int64_t)n_mat, kBoundsTexel)], a.texels, a.n_texels,
                              p1, o1, level0);
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

// pbr_resolve_materials_mip: resolve_materials_kernel's tile, accesses and record paths around the trilinear sampler;
// what is added is the footprint exchange between the loads and the resolve.
template <bool VEC>
__global__ __launch_bounds__(256) void resolve_materials_mip_kernel(const ResolveMipArgs ma) {
    using namespace resolve;
    const ResolveArgs& a = ma.r;
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
    // Every lane of the wave gets here together (pixels outside the frame and background pixels included), ahead of
    // the divergent branches below: the wave's two rows exchange u, v and the ids.
    Footprint d[2];
    quad_footprints(p0, p1, id0, id1, d);

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
            if (g0) resolve_pixel(m, a.texels, a.n_texels, p0, o0, trilinear(ma, first, d[0]));
            if (g1) resolve_pixel(m, a.texels, a.n_texels, p1, o1, trilinear(ma, first, d[1]));
        } else {
            if (g0)
                resolve_pixel(a.table[PBR_BOUNDS((int64_t)id0, (int64_t)n_mat, kBoundsTexel)], a.texels, a.n_texels,
                              p0, o0, trilinear(ma, id0, d[0]));
            if (g1)
                resolve_pixel(a.table[PBR_BOUNDS((int64_t)id1, (int64_t)n_mat, kBoundsTexel)], a.texels, a.n_texels,
                              p1, o1, trilinear(ma, id1, d[1]));
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

// pbr_resolve_materials_aniso: resolve_materials_mip_kernel with the anisotropic sampler. Written out again, not
// shared through a template, so that the older kernels' instruction streams stay what they were; the footprint
// exchange sits where it does there, ahead of every divergent branch, and is the only cross-lane traffic besides the
// one-material ballot. Left to itself the allocator takes 168 VGPRs, the most that three waves per SIMD allow (and took
// 172, two waves, for an earlier form of the sampler); the kernel names the three waves it is meant to keep -- the
// trilinear kernel's occupancy -- and gets 163 VGPRs without scratch.
template <bool VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3)))
void resolve_materials_aniso_kernel(const ResolveAnisoArgs aa) {
    using namespace resolve;
    const ResolveArgs& a = aa.m.r;
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
    // Every lane of the wave gets here together (pixels outside the frame and background pixels included), ahead of
    // the divergent branches below: the wave's two rows exchange u, v and the ids.
    Footprint d[2];
    quad_footprints(p0, p1, id0, id1, d);

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
            if (g0) resolve_pixel(m, a.texels, a.n_texels, p0, o0, anisotropic(aa, first, d[0]));
            if (g1) resolve_pixel(m, a.texels, a.n_texels, p1, o1, anisotropic(aa, first, d[1]));
        } else {
            if (g0)
                resolve_pixel(a.table[PBR_BOUNDS((int64_t)id0, (int64_t)n_mat, kBoundsTexel)], a.texels, a.n_texels,
                              p0, o0, anisotropic(aa, id0, d[0]));
            if (g1)
                resolve_pixel(a.table[PBR_BOUNDS((int64_t)id1, (int64_t)n_mat, kBoundsTexel)], a.texels, a.n_texels,
                              p1, o1, anisotropic(aa, id1, d[1]));
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

// One level of every chain that has it (pbr_generate_mips): a lane per texel of the level, its texture
// found from the prefix of texel counts; each byte channel is (a + b + c + d + 2) >> 2 of the 2 x 2 texels of the
// level before, columns and rows clamped to its last. Even and odd bytes are summed in 16-bit fields of two dwords
// (a sum is at most 1022).
__global__ __launch_bounds__(256) void generate_mip_level_kernel(const MipGenArgs a) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.n_out) return;
    int lo = 0, hi = a.n;  // the largest i with gen[i].first <= g
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.gen[PBR_BOUNDS((int64_t)mid, (int64_t)a.n, kBoundsTexel)].first <= g)
            lo = mid;
        else
            hi = mid;
    }
    const MipGen t = a.gen[PBR_BOUNDS((int64_t)lo, (int64_t)a.n, kBoundsTexel)];
    const uint32_t k = g - t.first;
    const int x = (int)(k % (uint32_t)t.dw), y = (int)(k / (uint32_t)t.dw);
    const int x0 = 2 * x, x1 = x0 + 1 < t.sw ? x0 + 1 : t.sw - 1, y0 = 2 * y, y1 = y0 + 1 < t.sh ? y0 + 1 : t.sh - 1;
    auto src = [&](int ty, int tx) {
        return a.src[PBR_BOUNDS((int64_t)t.src + (int64_t)(ty * t.sw + tx), a.n_src, kBoundsTexel)];
    };
    const uint32_t t00 = src(y0, x0), t10 = src(y0, x1), t01 = src(y1, x0), t11 = src(y1, x1);
    constexpr uint32_t kEven = 0x00FF00FFu, kHalf = 0x00020002u;
    const uint32_t even = (t00 & kEven) + (t10 & kEven) + (t01 & kEven) + (t11 & kEven) + kHalf;
    const uint32_t odd = ((t00 >> 8) & kEven) + ((t10 >> 8) & kEven) + ((t01 >> 8) & kEven) + ((t11 >> 8) & kEven) + kHalf;
    a.dst[PBR_BOUNDS((int64_t)t.dst + (int64_t)k, a.n_dst, kBoundsTexel)] = ((even >> 2) & kEven) | (((odd >> 2) & kEven) << 8);
}

hipError_t launch_generate_mip_level(const MipGenArgs& a, hipStream_t stream) {
    if (a.n <= 0 || a.n_out == 0) return hipSuccess;
    hipLaunchKernelGGL(generate_mip_level_kernel, dim3((a.n_out + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_resolve_materials_mip(const ResolveMipArgs& a, hipStream_t stream) {
    if (a.r.width <= 0 || a.r.height <= 0) return hipSuccess;
    const dim3 grid((a.r.width + kResolveTileW - 1) / kResolveTileW, (a.r.height + kResolveTileH - 1) / kResolveTileH);
    if (a.r.vec)
        hipLaunchKernelGGL((resolve_materials_mip_kernel<true>), grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((resolve_materials_mip_kernel<false>), grid, dim3(256), 0, stream, a);
    return hipGetLastError();
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

hipError_t launch_resolve_materials_aniso(const ResolveAnisoArgs& a, hipStream_t stream) {
    const ResolveArgs& r = a.m.r;
    if (r.width <= 0 || r.height <= 0) return hipSuccess;
    const dim3 grid((r.width + kResolveTileW - 1) / kResolveTileW, (r.height + kResolveTileH - 1) / kResolveTileH);
    if (r.vec)
        hipLaunchKernelGGL((resolve_materials_aniso_kernel<true>), grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((resolve_materials_aniso_kernel<false>), grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pbr
