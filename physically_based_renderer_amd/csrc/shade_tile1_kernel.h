// shade_tile1_kernel.h -- one pixel per work-item (32x8 tiles).
//
// The pair kernels' algorithm on the scalar fast path (pbr_device_math.h), with the lights staged through LDS and
// culled per workgroup (stage_chunk). Packing a pixel pair (shade_tile_kernel.h, shade_lean_kernel.h) halves
// the instruction count but not the VALU cycles (a v_pk_fma_f32 issues in twice the cycles of a
// v_fma_f32 on gfx950), and its register footprint costs a wave per SIMD; the launcher picks the
// faster layout (PBR_PIXELS_PER_THREAD).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "shade_common.h"
#include "shade_light_loops.h"
#include "shade_pixel.h"

namespace pbr {
namespace {

constexpr int kTileW1 = 32;

template <bool CULL>
__device__ __forceinline__ f3 lighting_fast1(const PixelInvariants& q, f3 pos, const float4* __restrict__ lights,
                                             const PassArgs& ps, Lds& s, const TileBounds& tb, bool cull_enabled,
                                             bool& redo, int& kept_total) {
    f3 direct = mk3(0.0f, 0.0f, 0.0f);
    for (int base = 0; base < ps.n_dir; base += kChunk) {  // directional: never culled
        const int cnt = min(kChunk, ps.n_dir - base);
        __syncthreads();
        stage_chunk<false>(lights, base, cnt, s, tb, false, true);
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float4* r = &s.light[3 * j];
            bool ok = q.fast_ok && r[2].w != 0.0f;
            const f3 c = directional_light<true>(q, r[0], r[1], ok);
            redo = redo || !ok;
            direct = add3(direct, c);  // shadowFactor (1,1,1) * c == c
        }
    }
    const int pt_begin = ps.n_dir, sp_begin = ps.n_dir + ps.n_point, end = sp_begin + ps.n_spot;
#pragma unroll 1
    for (int kind = 1; kind <= 2; ++kind) {
        const int b0 = kind == 1 ? pt_begin : sp_begin, b1 = kind == 1 ? sp_begin : end;
        for (int base = b0; base < b1; base += kChunk) {
            const int cnt = min(kChunk, b1 - base);
            __syncthreads();
            const int kept = stage_chunk<CULL>(lights, base, cnt, s, tb, cull_enabled, false);
            __syncthreads();
            kept_total += kept;
            for (int j = 0; j < kept; ++j) {
                const float4* r = &s.light[3 * j];
                bool ok = q.fast_ok && r[2].w != 0.0f;
                f3 c;
                const bool lit = kind == 1 ? point_or_spot_light<false, true>(q, pos, r[0], r[1], r[2], c, ok)
                                           : point_or_spot_light<true, true>(q, pos, r[0], r[1], r[2], c, ok);
                if (lit) {  // an unlit light adds +0 in the reference: the identity on this sum
                    redo = redo || !ok;
                    direct = add3(direct, c);
                }
            }
        }
    }
    return direct;
}

}  // namespace

template <int AMBIENT, bool F0_PLANE, bool APPLY_AO, bool CULL>
__global__ __launch_bounds__(kBlock) void shade_tile1_kernel(GBufferArgs gb, PassArgs ps,
                                                             const float4* __restrict__ lights,
                                                             const float4* __restrict__ env, FrameArgs fr,
                                                             int32_t* __restrict__ tile_kept,
                                                             bool exact_only) {
    __shared__ Lds s;
    load_libm_tables<AMBIENT == kAmbientIblDiffuse, kBlock>();  // powf (+ atanf with IBL) tables -> LDS (pbr_device_math.h)
    __syncthreads();
    const int tid = threadIdx.x;
    const int x = blockIdx.x * kTileW1 + (tid & (kTileW1 - 1));
    const int y = blockIdx.y * kTileH + (tid / kTileW1);
    const bool valid = (x < gb.width) && (y < gb.height);
    const int64_t idx = PBR_BOUNDS_PIXEL(valid ? (int64_t)y * gb.row_stride + x : 0, gb.width, gb.height, gb.row_stride,
                                         1, kBoundsGBuffer);  // frames are never empty here
    const bool geom = valid && is_geometry(fr, x, y);
    const bool any_geometry = fr.coverage == nullptr || __syncthreads_or(geom);

    f3 pos, n, albedo, f0;
    pos = mk3(gb.plane[0][idx], gb.plane[1][idx], gb.plane[2][idx]);
    n = mk3(gb.plane[3][idx], gb.plane[4][idx], gb.plane[5][idx]);
    albedo = mk3(gb.plane[6][idx], gb.plane[7][idx], gb.plane[8][idx]);
    const float metallic = gb.plane[9][idx];
    const float roughness = gb.plane[10][idx];
    const float ao = APPLY_AO ? gb.plane[11][idx] : 1.0f;
    if (F0_PLANE) {  // Default.hlsl:92
        f0 = mk3(gb.plane[12][idx], gb.plane[13][idx], gb.plane[14][idx]);
    } else {  // F0 = lerp(g_FresnelR0, diffuseAlbedo, metallic)  (Default.hlsl:94-95)
        f0 = mk3(hlerp(ps.fresnel_r0[0], albedo.x, metallic), hlerp(ps.fresnel_r0[1], albedo.y, metallic),
                 hlerp(ps.fresnel_r0[2], albedo.z, metallic));
    }
    // V = normalize(g_CameraPosW - pin.PosW)  (Default.hlsl:53)
    const f3 eye = mk3(ps.eye[0], ps.eye[1], ps.eye[2]);
    PixelInvariants q = make_invariants(n, normalize3(sub3(eye, pos)), albedo, f0, metallic, roughness);
    q.fast_ok = !exact_only && ps.eye_ok && fast_window_ok(pos, n, albedo, f0, metallic, roughness);

    TileBounds tb{};
    bool cull_enabled = false;
    if (CULL) {
        const bool finite = !geom || (isfinite(pos.x) && isfinite(pos.y) && isfinite(pos.z));
        const float big = 3.0e38f;
        float b[6] = {geom ? pos.x : big,  geom ? pos.y : big,  geom ? pos.z : big,
                      geom ? pos.x : -big, geom ? pos.y : -big, geom ? pos.z : -big};
#pragma unroll
        for (int i = 0; i < 3; ++i) b[i] = wave_min(b[i]);
#pragma unroll
        for (int i = 3; i < 6; ++i) b[i] = wave_max(b[i]);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) s.bounds[tid >> 6][i] = b[i];
        }
        cull_enabled = __syncthreads_and(finite) != 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            tb.mn[i] = fminf(fminf(s.bounds[0][i], s.bounds[1][i]), fminf(s.bounds[2][i], s.bounds[3][i]));
            tb.mx[i] = fmaxf(fmaxf(s.bounds[0][i + 3], s.bounds[1][i + 3]), fmaxf(s.bounds[2][i + 3], s.bounds[3][i + 3]));
        }
    }

    int kept_total = 0;
    bool redo = false;
    f3 direct = mk3(0.0f, 0.0f, 0.0f);
    if (any_geometry) direct = lighting_fast1<CULL>(q, pos, lights, ps, s, tb, cull_enabled, redo, kept_total);
    const bool need = geom && redo;
    const int n_exact = __syncthreads_count(need);
    if (n_exact != 0) {  // block-uniform: rare (edge inputs, EXACT_ONLY)
        f3 e, unused;
        lighting_exact<CULL>(q, q, pos, pos, need, false, lights, ps, s, tb, cull_enabled, e, unused);
        if (need) direct = e;
    }
    const int geo_px = __syncthreads_count(geom);
    if (tid == 0 && tile_kept != nullptr) {  // this layout culls per block (32x8 pixels)
        const int64_t t = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        int32_t* st = tile_kept + kStatsPerBlock * t;
        st[kStatCullKept] = CULL && any_geometry ? kept_total : 0;
        st[kStatCullTiles] = CULL && any_geometry ? 1 : 0;
        st[kStatExactPixels] = n_exact;
        st[kStatLightTerms] = any_geometry ? (ps.n_dir + (CULL ? kept_total : ps.n_point + ps.n_spot)) * geo_px : 0;
        st[kStatGeometryPixels] = geo_px;
        st[kStatBackfaceTests] = 0;
    }
    if (valid) {
        float4 c = geom ? finish_pixel<AMBIENT, APPLY_AO>(q, ao, direct, ps, env, q.fast_ok)
                        : sky_pixel(q.n, ps, fr.sky, !exact_only);
        if (!geom || alpha_keep(gb, idx, c)) store_pixel(fr, (int64_t)y * fr.out_stride + x, c);
    }
}

}  // namespace pbr
