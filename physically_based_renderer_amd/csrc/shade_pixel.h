// shade_pixel.h -- a pixel pair outside the light loops: the G-buffer load (load_pair), the BRDF invariants, the
// finish (ambient term or diffuse IBL, AO, Reinhard, gamma: Default.hlsl:139-160), the sky pass, the alpha test and
// the stores; and the exact re-pass of single pixels, which reads a pixel back and shades it from load to finish
// with the compiler's IEEE sequences (shade_pixel_exact, repass_exact).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pbr_unorm.h"
#include "shade_common.h"
#include "shade_light_loops.h"

namespace pbr {
namespace {

// The pair's G-buffer values in packed form: element 0 = pixel A, element 1 = pixel B.
struct PairIn {
    f3x2 pos, n, albedo, f0;
    v2 metallic, roughness, ao;
};

template <bool F0_PLANE, bool APPLY_AO>
__device__ __forceinline__ PairIn load_pair(const GBufferArgs& gb, const PassArgs& ps, int64_t ia, int64_t ib,
                                            bool vector_load) {
    v2 v[15];
    if (vector_load) {  // both pixels exist and the pair is 8-byte aligned in every plane
        ia = PBR_BOUNDS_PIXEL(ia, gb.width, gb.height, gb.row_stride, 2, kBoundsGBuffer);
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            if (i == 11 || (i >= 12 && !F0_PLANE)) continue;  // AO: read at the finish (load_ao_pair)
            const float2 t = *reinterpret_cast<const float2*>(gb.plane[i] + ia);
            v[i] = v2{t.x, t.y};
        }
    } else {
        PBR_COLD("scalar_loads");
        ia = PBR_BOUNDS_PIXEL(ia, gb.width, gb.height, gb.row_stride, 1, kBoundsGBuffer);
        ib = PBR_BOUNDS_PIXEL(ib, gb.width, gb.height, gb.row_stride, 1, kBoundsGBuffer);
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            if (i == 11 || (i >= 12 && !F0_PLANE)) continue;  // AO: read at the finish (load_ao_pair)
            v[i] = v2{gb.plane[i][ia], gb.plane[i][ib]};
        }
    }
    PairIn p;
    p.pos = f3x2{v[0], v[1], v[2]};
    p.n = f3x2{v[3], v[4], v[5]};
    p.albedo = f3x2{v[6], v[7], v[8]};
    p.metallic = v[9];
    p.roughness = v[10];
    p.ao = splat(1.0f);  // PBR_FLAG_APPLY_AO: load_ao_pair after the light loop
    if (F0_PLANE) {  // Default.hlsl:92
        p.f0 = f3x2{v[12], v[13], v[14]};
    } else {  // F0 = lerp(g_FresnelR0, diffuseAlbedo, metallic)  (Default.hlsl:94-95): x + s*(y - x)
        p.f0 = f3x2{ps.fresnel_r0[0] + p.metallic * (p.albedo.x - ps.fresnel_r0[0]),
                    ps.fresnel_r0[1] + p.metallic * (p.albedo.y - ps.fresnel_r0[1]),
                    ps.fresnel_r0[2] + p.metallic * (p.albedo.z - ps.fresnel_r0[2])};
    }
    return p;
}

// An optimisation barrier on the pair's raw values: the compiler must assume they changed, so a computation
// from them after this point is not merged with the same computation before it. No instructions.
__device__ __forceinline__ void launder(v2& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void launder(f3x2& x) {
    launder(x.x);
    launder(x.y);
    launder(x.z);
}
[[maybe_unused]] __device__ __forceinline__ void launder(PairIn& p) {
    launder(p.pos);
    launder(p.n);
    launder(p.albedo);
    launder(p.f0);
    launder(p.metallic);
    launder(p.roughness);
    launder(p.ao);
}

// V = normalize(g_CameraPosW - pin.PosW) (Default.hlsl:53) and the BRDF invariants of the pair. In the window
// every component of eye - pos is 0 or >= 2^-44 and |eye - pos| < 2^22, so the exact fast normalize applies
// once |V| >= 2^-30; other pixels take the IEEE sequences.
__device__ __forceinline__ f3x2 pair_view(const PairIn& p, const PassArgs& ps, m2 fast2) {
    const f3x2 ve = f3x2{ps.eye[0] - p.pos.x, ps.eye[1] - p.pos.y, ps.eye[2] - p.pos.z};
    m2 okv = fast2;
    f3x2 v = normalize_x2(ve, okv);
    const bool va_ok = on(okv.x), vb_ok = on(okv.y);
    if (__builtin_expect(!(va_ok && vb_ok), 0)) {
        PBR_COLD("v_ieee");
        const f3 v0 = va_ok ? lane(v, 0) : normalize3(lane(ve, 0)), v1 = vb_ok ? lane(v, 1) : normalize3(lane(ve, 1));
        v = f3x2{v2{v0.x, v1.x}, v2{v0.y, v1.y}, v2{v0.z, v1.z}};
    }
    return v;
}
__device__ __forceinline__ PixelInvariants2 pair_invariants(const PairIn& p, const PassArgs& ps, m2 fast2) {
    return make_invariants(p.n, pair_view(p, ps, fast2), p.albedo, p.f0, p.metallic, p.roughness, fast2);
}
// Only what the finish reads (make_finish_invariants): the wave-balanced kernels after their light loop.
[[maybe_unused]] __device__ __forceinline__ PixelInvariants2 pair_finish_invariants(const PairIn& p, const PassArgs& ps, m2 fast2) {
    return make_finish_invariants(p.n, pair_view(p, ps, fast2), p.albedo, p.f0, p.metallic);
}

// Ambient + tonemap + gamma for one pixel (Default.hlsl:139-160), returns the output RGBA.
// Reinhard c / (c + 1) (Default.hlsl:153, Skybox.hlsl:47): the Markstein step when `fast` and c is 0 or
// in [2^-100, 2^60] (then c + 1 is in [1, 2^60]); the IEEE division otherwise.
__device__ __forceinline__ float reinhard(float c, bool fast) {
    if (fast && (c == 0.0f || (c >= 0x1p-100f && c <= 0x1p60f))) return div_nr(c, recip_nr(c + 1.0f));
    return c / (c + 1.0f);
}
// PBR_FLAG_FAITHFUL waves: Reinhard with the hardware reciprocal (c >= 0 here; inf / NaN give NaN as
// the IEEE quotient does) and the gamma encode of pow_inv_gamma_faithful. v_rcp_f32 returns 0 where
// the reciprocal is subnormal (c + 1 >= 2^126; measured on gfx950, tests/test_gpu_strength_range.py on the parent of
// the gate), which would make the pixel 0 where the quotient is ~1: the sum window (<= 2^100) and the host's bound on
// the constant ambient and on fp32 environment texels (pbr_context.hip, kFaithfulAmbientHi) keep c + 1 below 2^111
// without PBR_FLAG_APPLY_AO; with it, only while the AO plane's value is within 2^15 (not checked: DESIGN.md §2).
__device__ __forceinline__ float reinhard_faithful(float c) { return c * __builtin_amdgcn_rcpf(c + 1.0f); }

// The ambient term of Default.hlsl:139-150 (before the AO extension).
template <int AMBIENT>
__device__ __forceinline__ f3 ambient_term(const PixelInvariants& p, const PassArgs& ps, const float4* __restrict__ env) {
    const PixelInvariants& q = p;
    if (AMBIENT == kAmbientIblDiffuse) {
        // Default.hlsl:141-146: kS = FresnelSchlick(N, V, F0); kD = (1 - kS)(1 - metallic);
        // irradiance = env.Sample(linear-wrap, WorldToSkyUV(N)); ambient = kD * (irradiance * albedo)
        const float cos_theta = hsat(dot3(p.n, q.v));
        const float pw = pow5_glibc(1.0f - cos_theta);
        const f3 ks = mk3(p.f0.x + q.one_minus_f0.x * pw, p.f0.y + q.one_minus_f0.y * pw, p.f0.z + q.one_minus_f0.z * pw);
        const f3 kd = mk3((1.0f - ks.x) * q.one_minus_metal, (1.0f - ks.y) * q.one_minus_metal,
                          (1.0f - ks.z) * q.one_minus_metal);
        float su, sv;
        world_to_sky_uv(p.n, su, sv);
        const f3 irr = sample_linear_wrap(env, ps.env_w, ps.env_h, su, sv);
        const f3 diffuse = mk3(irr.x * p.albedo.x, irr.y * p.albedo.y, irr.z * p.albedo.z);
        return mk3(kd.x * diffuse.x, kd.y * diffuse.y, kd.z * diffuse.z);
    }
    // g_AmbientLight * diffuseAlbedo  (Default.hlsl:150)
    return mk3(ps.ambient[0] * p.albedo.x, ps.ambient[1] * p.albedo.y, ps.ambient[2] * p.albedo.z);
}

// The diffuse-IBL ambient of Default.hlsl:141-146 for both pixels of the pair in packed form: ambient_term's
// operations element for element (FresnelSchlick(N, V) with kD = (1 - kS)(1 - metallic), WorldToSkyUV through the
// branch-free pair forms of glibc's atan2f / asinf (libm_f32_x2.h, bit-identical), the linear-wrap env fetch per
// pixel, kD * irradiance * albedo). Faithful waves take the IBL Fresnel x^5 from pow5_faithful (<= 1 ulp from glibc
// off the grazing band x > 0.99, where it is glibc's: <= 1.2e-6 on kD); exact waves glibc's powf.
// Pixels whose normal has a component the pair forms do not cover (NaN, inf, nonzero magnitudes outside
// [2^-40, 2^40], |N.y| > 1) take the scalar functions. `live_a` / `live_b`: the elements whose result is used.
__device__ __forceinline__ f3x2 ambient_ibl_pair(const PixelInvariants2& q, const PassArgs& ps,
                                               const float4* __restrict__ env, bool faithful, bool live_a,
                                               bool live_b) {
    const v2 x = 1.0f - dot3_sat(q.n, q.v);  // 1 - saturate(dot(N, V)): the clamp bit maps NaN to 0 as hsat
    const v2 pw = faithful ? pow5_faithful(x, lanes(live_a || live_b)) : v2{pow5_glibc(x.x), pow5_glibc(x.y)};
    const f3x2 kd = f3x2{(1.0f - (q.f0.x + q.one_minus_f0.x * pw)) * q.one_minus_metal,
                         (1.0f - (q.f0.y + q.one_minus_f0.y * pw)) * q.one_minus_metal,
                         (1.0f - (q.f0.z + q.one_minus_f0.z * pw)) * q.one_minus_metal};
    // WorldToSkyUV (LightingUtil.hlsl:216-225): the main parts of the pair forms for every element; their patches
    // (a zero component, the exponent-gap shortcuts, |N.y| == 1) in one wave-uniform branch, only when an element
    // of the wave is odd; the scalar functions inside it for live special elements (libm_f32_x2.h).
    // `odd` is not masked by `live`: an element that is not live may hold anything, and only an element that is not
    // special has the bounded texel coordinates the branch-free wrap needs (pbr_device_math.h, wrap_sky_column), so
    // a wave with any special element, live or not, takes the general wrap.
    int oa[2], ob[2];
    v2 q_abs;
    const v2 az = pbr_atan2f_x2_head(q.n.z, q.n.x, oa, &q_abs, PBR_LIBM_ATAN_TAB, 1);
    v2 uy = pbr_asinf_x2_main(q.n.y, ob);
    v2 ux;
    bool any_special = false;  // wave-uniform
    if (__builtin_expect(lanes((oa[0] | ob[0] | oa[1] | ob[1]) != 0) != 0, 0)) {
        PBR_COLD("ibl_patch");
        int sa[2], sb[2];
        ux = pbr_atan2f_x2_tail_patch(q.n.z, q.n.x, q_abs, az);
        uy = pbr_asinf_x2_patch(q.n.y, uy, sb);
        pbr_atan2f_x2_special(q.n.z, q.n.x, sa);
        const bool sp_a = (sa[0] | sb[0]) != 0, sp_b = (sa[1] | sb[1]) != 0;
        any_special = lanes(sp_a || sp_b) != 0;
        const bool spec_a = live_a && sp_a, spec_b = live_b && sp_b;
        if (__builtin_expect(lanes(spec_a || spec_b) != 0, 0)) {
            PBR_COLD("ibl_special");
            if (spec_a) {
                ux.x = pbr_atan2f(q.n.z.x, q.n.x.x);
                uy.x = pbr_asinf(q.n.y.x);
            }
            if (spec_b) {
                ux.y = pbr_atan2f(q.n.z.y, q.n.x.y);
                uy.y = pbr_asinf(q.n.y.y);
            }
        }
    } else {
        ux = pbr_atan2f_x2_tail(q.n.z, q.n.x, az);
    }
    ux = ux * 0.1591f;
    uy = uy * 0.3183f;
    ux = ux + 0.5f;
    uy = uy + 0.5f;
    uy = 1.0f - uy;
    ux = 1.0f - ux;
    ux = ux + 0.25f;
    f3 ia, ib;
    if (__builtin_expect(any_special, 0)) {
        PBR_COLD("ibl_wrap_general");
        ia = sample_linear_wrap(env, ps.env_w, ps.env_h, ux.x, uy.x);
        ib = sample_linear_wrap(env, ps.env_w, ps.env_h, ux.y, uy.y);
    } else {
        ia = sample_linear_wrap<true>(env, ps.env_w, ps.env_h, ux.x, uy.x);
        ib = sample_linear_wrap<true>(env, ps.env_w, ps.env_h, ux.y, uy.y);
    }
    const f3x2 irr = f3x2{v2{ia.x, ib.x}, v2{ia.y, ib.y}, v2{ia.z, ib.z}};
    return f3x2{kd.x * (irr.x * q.albedo.x), kd.y * (irr.y * q.albedo.y), kd.z * (irr.z * q.albedo.z)};
}

// The rest of the PS from the ambient term: AO (extension), + direct, Reinhard, gamma (Default.hlsl:150-160).
template <bool APPLY_AO>
__device__ __forceinline__ float4 finish_lit(f3 ambient, float ao, f3 direct, const PassArgs& ps, bool fast,
                                             bool faithful) {
    if (APPLY_AO) ambient = mk3(ambient.x * ao, ambient.y * ao, ambient.z * ao);
    f3 lit = add3(ambient, direct);
    if (faithful) {  // wave-uniform
        lit = mk3(reinhard_faithful(lit.x), reinhard_faithful(lit.y), reinhard_faithful(lit.z));
        return make_float4(pow_inv_gamma_faithful(lit.x), pow_inv_gamma_faithful(lit.y),
                           pow_inv_gamma_faithful(lit.z), ps.opacity);
    }
    PBR_PHASE("xfinish");  // the exact finish (the faithful census stops here)
    lit = mk3(reinhard(lit.x, fast), reinhard(lit.y, fast), reinhard(lit.z, fast));  // Default.hlsl:153
    return make_float4(pow_inv_gamma(lit.x), pow_inv_gamma(lit.y), pow_inv_gamma(lit.z),
                       ps.opacity);
}

// The finish of both pixels of the pair (finish_pixel each): with the diffuse IBL, the ambient pair is formed in
// packed form first (ambient_ibl_pair); `live_a` / `live_b` say which elements are shaded geometry.
template <int AMBIENT, bool APPLY_AO>
__device__ __forceinline__ void finish_pair(const PixelInvariants2& q2, const PixelInvariants& ua,
                                            const PixelInvariants& ub, float ao_a, float ao_b, f3 da, f3 db,
                                            const PassArgs& ps, const float4* __restrict__ env, bool fast_a,
                                            bool fast_b, bool faithful, bool live_a, bool live_b, float4& ca,
                                            float4& cb) {
    if constexpr (AMBIENT == kAmbientIblDiffuse) {
        PBR_PHASE("ibl");
        const f3x2 amb = ambient_ibl_pair(q2, ps, env, faithful, live_a, live_b);
        PBR_PHASE("finish");
        if (live_a) ca = finish_lit<APPLY_AO>(lane(amb, 0), ao_a, da, ps, fast_a, faithful);
        if (live_b) cb = finish_lit<APPLY_AO>(lane(amb, 1), ao_b, db, ps, fast_b, faithful);
    } else {
        if (live_a) ca = finish_lit<APPLY_AO>(ambient_term<AMBIENT>(ua, ps, env), ao_a, da, ps, fast_a, faithful);
        if (live_b) cb = finish_lit<APPLY_AO>(ambient_term<AMBIENT>(ub, ps, env), ao_b, db, ps, fast_b, faithful);
    }
}

template <int AMBIENT, bool APPLY_AO>
__device__ __forceinline__ float4 finish_pixel(const PixelInvariants& p, float ao, f3 direct, const PassArgs& ps,
                                               const float4* __restrict__ env, bool fast, bool faithful = false) {
    return finish_lit<APPLY_AO>(ambient_term<AMBIENT>(p, ps, env), ao, direct, ps, fast, faithful);
}

// The sky pass for a background pixel (Skybox.hlsl:37-49): sampleCoord = normalize(PosW);
// WorldToSkyUV; g_SkyArray[0].Sample(linear-wrap); Reinhard; gamma; alpha 1. sky_colour is the sampled colour,
// sky_finish the rest.
__device__ __forceinline__ f3 sky_colour(f3 dir, const PassArgs& ps, const float4* __restrict__ sky) {
    const f3 c = normalize3(dir);
    float u, v;
    world_to_sky_uv(c, u, v);
    return sample_linear_wrap(sky, ps.sky_w, ps.sky_h, u, v);
}
__device__ __forceinline__ float4 sky_finish(f3 col, bool fast) {
    col = mk3(reinhard(col.x, fast), reinhard(col.y, fast), reinhard(col.z, fast));
    return make_float4(pow_inv_gamma(col.x), pow_inv_gamma(col.y), pow_inv_gamma(col.z),
                       1.0f);
}
__device__ __forceinline__ float4 sky_pixel(f3 dir, const PassArgs& ps, const float4* __restrict__ sky, bool fast) {
    PBR_COLD("sky");
    return sky_finish(sky_colour(dir, ps, sky), fast);
}

// unorm8: the D3D FLOAT -> UNORM8 rule of the R8G8B8A8_UNORM back buffer (pbr_unorm.h).
__device__ __forceinline__ void store_pixel(const FrameArgs& fr, int64_t off, float4 c) {
    off = PBR_BOUNDS_PIXEL(off, fr.width, fr.height, fr.out_stride, 1, kBoundsOutput);
    if (fr.format == kOutRgba8) {
        static_cast<uint32_t*>(fr.out)[off] = unorm8(c.x) | (unorm8(c.y) << 8) | (unorm8(c.z) << 16) | (unorm8(c.w) << 24);
    } else {
        static_cast<float4*>(fr.out)[off] = c;
    }
}

// PBR_FLAG_ALPHA_TEST, the reference's ALPHA_TEST permutation (Default.hlsl:111-113, alphaTestedPS): fragOpacity is
// the pixel's opacity-map value (G-buffer plane 15, index gidx) and clip(fragOpacity - 0.1f) discards the fragment
// when that is negative (NaN is not) -- the pixel's output is then left untouched; otherwise fragOpacity is the
// output alpha (Default.hlsl:160). Geometry pixels only (the sky PS has no clip). Returns whether to store.
__device__ __forceinline__ bool alpha_keep(const GBufferArgs& gb, int64_t gidx, float4& c) {
    if (!gb.alpha_test) return true;  // uniform
    const float op = gb.plane[15][PBR_BOUNDS_PIXEL(gidx, gb.width, gb.height, gb.row_stride, 1, kBoundsGBuffer)];
    if (op - 0.1f < 0.0f) return false;
    c.w = op;
    return true;
}

// alpha_keep for the pixel pair at G-buffer row offset `grow` (ga / gb_: geometry), in one uniform branch that
// passes without the flag: the stores of an ordinary pass see no extra work or live values.
__device__ __forceinline__ void alpha_keep_pair(const GBufferArgs& gb, int64_t grow, bool ga, bool gb_, float4& ca,
                                                float4& cb, bool& keep_a, bool& keep_b) {
    keep_a = keep_b = true;
    if (__builtin_expect(gb.alpha_test, 0)) {
        PBR_COLD("alpha");
        if (ga) keep_a = alpha_keep(gb, grow, ca);
        if (gb_) keep_b = alpha_keep(gb, grow + 1, cb);
    }
}

// Coverage of a pixel: geometry unless the frame has a coverage plane holding 0 there.
__device__ __forceinline__ bool is_geometry(const FrameArgs& fr, int x, int y) {
    return fr.coverage == nullptr ||
           fr.coverage[PBR_BOUNDS_PIXEL((int64_t)y * fr.coverage_stride + x, fr.width, fr.height, fr.coverage_stride, 1,
                                        kBoundsCoverage)] != 0;
}

// The lane's index in its wave, from the hardware (v_mbcnt) in volatile asm: the compiler can neither CSE it
// with an earlier value nor hoist it, so the pair kernel re-derives its pixel coordinates at the store
// instead of keeping the 64-bit output offset live across the light loops (at the 128-VGPR cap of 4 waves
// per SIMD that offset was spilled to scratch: 8 bytes written and re-read per work-item).
__device__ __forceinline__ int lane_id_fresh() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

}  // namespace

// One pixel (G-buffer index `idx`) with the compiler's IEEE sequences: V, the BRDF invariants, the light sum in
// the reference's order (lighting_exact_wave: every light, no culling) and the finish (faithful_finish: the
// faithful wave's finish of a re-passed pixel). Wave-uniform call; lanes with !need return zeros.
// LANES: `idx` is wave-uniform and the lanes split the lights (lighting_exact_lanes); otherwise every lane with
// `need` shades its own pixel.
template <int AMBIENT, bool F0_PLANE, bool APPLY_AO, bool LANES>
__device__ __forceinline__ float4 shade_pixel_exact(const GBufferArgs& gb, const PassArgs& ps,
                                                    const float4* __restrict__ lights, const float4* __restrict__ env,
                                                    int64_t idx, bool need, bool faithful_finish) {
    if (!LANES) idx = need ? idx : 0;
    idx = PBR_BOUNDS_PIXEL(idx, gb.width, gb.height, gb.row_stride, 1, kBoundsGBuffer);
    const f3 pos = mk3(gb.plane[0][idx], gb.plane[1][idx], gb.plane[2][idx]);
    const f3 n = mk3(gb.plane[3][idx], gb.plane[4][idx], gb.plane[5][idx]);
    const f3 albedo = mk3(gb.plane[6][idx], gb.plane[7][idx], gb.plane[8][idx]);
    const float metallic = gb.plane[9][idx], roughness = gb.plane[10][idx];
    const float ao = APPLY_AO ? gb.plane[11][idx] : 1.0f;
    // F0 exactly as load_pair forms it (Default.hlsl:92-95).
    const f3 f0 = F0_PLANE ? mk3(gb.plane[12][idx], gb.plane[13][idx], gb.plane[14][idx])
                           : mk3(ps.fresnel_r0[0] + metallic * (albedo.x - ps.fresnel_r0[0]),
                                 ps.fresnel_r0[1] + metallic * (albedo.y - ps.fresnel_r0[1]),
                                 ps.fresnel_r0[2] + metallic * (albedo.z - ps.fresnel_r0[2]));
    const f3 eye = mk3(ps.eye[0], ps.eye[1], ps.eye[2]);
    const PixelInvariants q = make_invariants(n, normalize3(sub3(eye, pos)), albedo, f0, metallic, roughness);
    f3 d, unused;
    if (LANES)
        d = lighting_exact_lanes(q, pos, lights, ps);
    else
        lighting_exact_wave(q, q, pos, pos, need, false, lights, ps, d, unused);
    return finish_pixel<AMBIENT, APPLY_AO>(q, ao, d, ps, env, false, faithful_finish);
}

// A wave re-passes up to this many pixels one at a time with the lanes splitting the lights (each costs about
// one light's IEEE sequence plus the ordered adds); more, and every lane takes its own pixels.
constexpr int kLanesRepassMax = 8;

// The exact re-pass of one wave's pixels (need_a / need_b: the pair's elements), after the wave has stored
// everything else: each pixel is read back from the G-buffer and evaluated with the IEEE sequences
// (shade_pixel_exact; `faithful`: the finish of a faithful wave), so nothing of the fast path is live here.
// Up to kLanesRepassMax pixels go one at a time with the lanes splitting the lights; more, and every lane
// takes its own pixels.
template <int AMBIENT, bool F0_PLANE, bool APPLY_AO>
__device__ __forceinline__ void repass_exact(const GBufferArgs& gb, const PassArgs& ps,
                                             const float4* __restrict__ lights, const float4* __restrict__ env,
                                             const FrameArgs& fr, int tile_x, int tile_y, int wave_id, bool need_a,
                                             bool need_b, int n_exact, bool faithful) {
    const int tid = threadIdx.x & 63;
    if (n_exact <= kLanesRepassMax) {
        uint64_t ma = lanes(need_a), mb = lanes(need_b);
        while ((ma | mb) != 0) {
            const bool second = ma == 0;
            uint64_t& m = second ? mb : ma;
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            const int rx = tile_x * kTileW + 2 * (l & 31) + (second ? 1 : 0);
            const int ry = tile_y * kTileH + 2 * wave_id + (l >> 5);
            float4 c = shade_pixel_exact<AMBIENT, F0_PLANE, APPLY_AO, true>(gb, ps, lights, env,
                                                                            (int64_t)ry * gb.row_stride + rx, true,
                                                                            faithful);
            if (tid == 0 && alpha_keep(gb, (int64_t)ry * gb.row_stride + rx, c))
                store_pixel(fr, (int64_t)ry * fr.out_stride + rx, c);
        }
    } else {
        const int ln = lane_id_fresh();
        const int rx = tile_x * kTileW + 2 * (ln & 31);
        const int ry = tile_y * kTileH + 2 * wave_id + (ln >> 5);
        const int64_t gi = (int64_t)ry * gb.row_stride + rx, oi = (int64_t)ry * fr.out_stride + rx;
        if (lanes(need_a) != 0) {
            float4 c = shade_pixel_exact<AMBIENT, F0_PLANE, APPLY_AO, false>(gb, ps, lights, env, gi, need_a, faithful);
            if (need_a && alpha_keep(gb, gi, c)) store_pixel(fr, oi, c);
        }
        if (lanes(need_b) != 0) {
            float4 c = shade_pixel_exact<AMBIENT, F0_PLANE, APPLY_AO, false>(gb, ps, lights, env, gi + 1, need_b,
                                                                             faithful);
            if (need_b && alpha_keep(gb, gi + 1, c)) store_pixel(fr, oi + 1, c);
        }
    }
}

}  // namespace pbr
