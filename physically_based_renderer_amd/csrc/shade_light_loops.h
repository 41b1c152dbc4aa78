// shade_light_loops.h -- the light loops of the shading kernels: ComputeLighting (LightingUtil.hlsl:170-200).
//
// Lights: the pair kernels read each light record (3 float4 = the reference's 48-byte `Light`,
// LightingUtil.hlsl:9-17) with wave-uniform scalar loads; nothing is staged and the light loop has no
// barrier. Tiled culling (PBR_FLAG_TILED_CULLING) is per wave: the wave's 64x2-pixel world-space box
// (wave64 butterflies), one range test per lane and light, and the ballot of the survivors walked in
// order. A light is dropped only when it is provably beyond the 100-unit range of every pixel of the
// wave, so the reference loop (LightingUtil.hlsl:131) would have added +0 for it: the culled result
// is bit-identical to the unculled one. (The one-pixel kernel, shade_tile1_kernel.h, stages lights through LDS
// with stage_chunk and culls per workgroup, with an in-order ballot + mbcnt compaction.)
//
// Exact fallback: a pixel whose inputs or intermediates leave the fast-path window for any light is
// flagged; after the fast loop, a wave (one-pixel kernel: a block) with any flagged pixel re-runs the light loop
// for those pixels with the compiler's full IEEE sequences (scalar, pbr_device_math.h), replacing their sums:
// lighting_exact (staged, per block), lighting_exact_wave (per wave), lighting_exact_lanes (one pixel per wave).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "shade_common.h"

namespace pbr {
namespace {

// Stage lights [begin, begin+count) of the global list into LDS, culled against the tile when CULL.
// Returns the number staged (identical in every work-item). Caller brackets with barriers.
// Each staged record is the 48-byte Light with its unused pad1 (.w of the position float4)
// replaced by the light's fast-path window flag (pbr_device_math.h, light_window_ok).
template <bool CULL>
__device__ __forceinline__ int stage_chunk(const float4* __restrict__ lights, int begin, int count, Lds& s,
                                           const TileBounds& tb, bool cull_enabled, bool directional) {
    const int tid = threadIdx.x;
    const bool have = tid < count;
    float4 l0 = make_float4(0.f, 0.f, 0.f, 0.f), l1 = l0, l2 = l0;
    if (have) {
        const float4* src = lights + 3 * (begin + tid);
        l0 = src[0];
        l1 = src[1];
        l2 = src[2];
        l2.w = light_window_ok(directional, l1, l2) ? 1.0f : 0.0f;
    }
    if (!CULL) {
        if (have) {
            s.light[3 * tid + 0] = l0;
            s.light[3 * tid + 1] = l1;
            s.light[3 * tid + 2] = l2;
        }
        return count;
    }
    bool keep = have;
    if (have && cull_enabled) {
        float dx = hmax(hmax(tb.mn[0] - l2.x, l2.x - tb.mx[0]), 0.0f);
        float dy = hmax(hmax(tb.mn[1] - l2.y, l2.y - tb.mx[1]), 0.0f);
        float dz = hmax(hmax(tb.mn[2] - l2.z, l2.z - tb.mx[2]), 0.0f);
        keep = (dx * dx + dy * dy + dz * dz) <= kCullRadius * kCullRadius;
    }
    const uint64_t mask = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
    if (lane == 0) s.wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        const int c = s.wave_cnt[w];
        off += (w < wave) ? c : 0;
        total += c;
    }
    if (keep) {
        const int slot = off + before;
        s.light[3 * slot + 0] = l0;
        s.light[3 * slot + 1] = l1;
        s.light[3 * slot + 2] = l2;
    }
    return total;
}

// Light j's record as uploaded (the reference's 48-byte Light; pbr_set_pass stores the light's
// fast-path window flag in the unused pad1 = .w of the position). The index is wave-uniform, so
// these are scalar loads through the scalar cache: no LDS staging, no barrier.
struct LightRec {
    float4 s, d, p;
};
__device__ __forceinline__ LightRec light_rec(const float4* __restrict__ lights, int j, const PassArgs& ps) {
    j = PBR_BOUNDS(j, ps.n_dir + ps.n_point + ps.n_spot, kBoundsLight);
    return LightRec{lights[3 * j], lights[3 * j + 1], lights[3 * j + 2]};
}
// The light's fast-path window flag (pbr_set_pass writes 1.0f or 0.0f into pad1) as a lane mask, on
// the scalar unit: the record is in SGPRs, so an integer test of its bits needs no VALU compare.
__device__ __forceinline__ m2 light_flag(const LightRec& r) {
    const uint64_t m = (__float_as_uint(r.p.w) << 1) != 0u ? ~0ull : 0ull;
    return m2{m, m};
}

// The tiled-culling range test: point/spot light `lp` may be within range of some point of the box `wb`
// (the box distance against the conservative radius kCullRadius).
__device__ __forceinline__ bool light_survives(float4 lp, const TileBounds& wb) {
    const float dx = hmax(hmax(wb.mn[0] - lp.x, lp.x - wb.mx[0]), 0.0f);
    const float dy = hmax(hmax(wb.mn[1] - lp.y, lp.y - wb.mx[1]), 0.0f);
    const float dz = hmax(hmax(wb.mn[2] - lp.z, lp.z - wb.mx[2]), 0.0f);
    return (dx * dx + dy * dy + dz * dz) <= kCullRadius * kCullRadius;
}

// The number of light terms the wave sums under tiled culling: directional lights + the point/spot lights
// that survive its box (one lane per light, the same test as the loop). PBR_FLAG_FAITHFUL's bound counts
// summed terms, so a culled pass with more lights than the bound allows can still run it per wave.
// The survivor masks of lights [base, base + 256) of the range [.., b1): bit l of m[k] = light base + 64 k + l
// may reach the wave's box. The four chunks' position loads are issued together before any test (a dependent load
// per 64 lights left the wave waiting for each in turn: config 4's per-wave term count and culled walk).
__device__ __forceinline__ void survivor_masks(const float4* __restrict__ lights, int base, int b1,
                                               const TileBounds& wb, bool cull_enabled, uint64_t (&m)[4]) {
    const int lane = (int)(threadIdx.x & 63);
    float4 lp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = base + 64 * k + lane;
        lp[k] = j < b1 && cull_enabled ? lights[3 * j + 2] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = base + 64 * k + lane;
        m[k] = lanes(j < b1 && (!cull_enabled || light_survives(lp[k], wb)));
    }
}

// The survivor masks of the first 256 point lights as wave_light_terms found them, for the culled walk to reuse
// (valid: a pass without spot lights, whose walk over the point lights starts with the same range and box).
struct FirstSurvivors {
    uint64_t m[4];
    bool valid = false;
};
__device__ __forceinline__ int wave_light_terms(const float4* __restrict__ lights, const PassArgs& ps,
                                                const TileBounds& wb, bool cull_enabled,
                                                FirstSurvivors* first = nullptr) {
    const int b0 = ps.n_dir, b1 = ps.n_dir + ps.n_point + ps.n_spot;
    if (!cull_enabled) return b1;
    int total = ps.n_dir;
    for (int base = b0; base < b1; base += 256) {
        uint64_t m[4];
        if (first != nullptr && first->valid && base == b0) {  // found already (lean_wave's early survivors)
            for (int k = 0; k < 4; ++k) m[k] = first->m[k];
        } else {
            survivor_masks(lights, base, b1, wb, true, m);
            if (first != nullptr && base == b0 && ps.n_spot == 0) {
                for (int k = 0; k < 4; ++k) first->m[k] = m[k];
                first->valid = true;
            }
        }
        total += __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
    }
    return total;
}

// ComputeLighting (LightingUtil.hlsl:170-200) for both pixels of the pair on the packed fast path:
// in-order sum from +0; `redo` collects pixels that left the fast-path window for a lit light.
// LEAN (wave-uniform): the wave's pixels satisfy the extra conditions of brdf_x2<true>.
// CULL: wave-level tiled culling. Each round, lane l range-tests point/spot light base + l against
// the wave's own world-space box `wb` (its 64x2 pixels); the ballot of the survivors is walked in
// increasing bit order, so the kept lights are summed in the reference's order. A dropped light is
// one the reference's `d > 100` test (LightingUtil.hlsl:131) rejects for every pixel of the wave, i.e.
// a +0 term: the result is bit-identical to the unculled pass.
// BALANCED (untiled faithful lean waves, ps.balanced): the point lights run through the back-face-rejected,
// wave-balanced lists of pbr_balanced.h (region `bal`; `geo_a` / `geo_b`: the pair's geometry pixels).
template <bool CULL, bool LEAN, bool FAITHFUL = false, bool BALANCED = false>
__device__ __forceinline__ f3x2 lighting_fast(const PixelInvariants2& q, const f3x2& pos, m2 fast_ok,
                                              const float4* __restrict__ lights, const PassArgs& ps,
                                              const TileBounds& wb, bool cull_enabled, m2& redo, int& kept_total,
                                              BalancedWaveLds* bal = nullptr, const float* bal_lights = nullptr,
                                              bool geo_a = false, bool geo_b = false, BalMasks bm = BalMasks{},
                                              unsigned long long* bal_prof = nullptr,
                                              const FirstSurvivors* first = nullptr) {
    f3x2 direct = splat3(0.0f, 0.0f, 0.0f);
    Faithful2 fi{};
    if (FAITHFUL) fi = make_faithful<!CULL>(q);
    // Exact balanced passes have no directional lights (host: PassArgs::balanced == 2): their loop is compiled
    // out there, it was the register peak of that path.
    const int n_dir = BALANCED && !FAITHFUL ? 0 : ps.n_dir;
    for (int j = 0; j < n_dir; ++j) {  // directional: never culled
        PBR_COLD("directional");
        const LightRec r = light_rec(lights, j, ps);
        m2 ok = fast_ok & light_flag(r);
        if (FAITHFUL) {
            directional_faithful_x2<LEAN, !CULL>(q, fi, r.s, r.d, ok, direct);
        } else {
            const f3x2 c = directional_x2<LEAN>(q, r.s, r.d, ok);
            direct = add3(direct, c);  // shadowFactor (1,1,1) * c == c
        }
        redo |= ~ok;
    }
    const int pt_begin = ps.n_dir, sp_begin = ps.n_dir + ps.n_point, end = sp_begin + ps.n_spot;
    // Point lights, then spot lights: one loop each (SPOT is a template constant, so the point loop
    // carries no spot code and no per-light branch on the kind).
    auto run_kind = [&](auto spot_tag, int b0, int b1) {
        constexpr bool SPOT = decltype(spot_tag)::value;
        auto point = [&](int j) {
            const LightRec r = light_rec(lights, j, ps);
            m2 ok = fast_ok & light_flag(r);
            // An unlit light adds +0 in the reference; here its lanes carry +-0 (zero attenuation)
            // when inside the window, and every lane outside it is redone.
            if (FAITHFUL) {
                point_or_spot_faithful_x2<SPOT, LEAN, !CULL>(q, fi, pos, r.s, r.d, r.p, ok, direct);
            } else {
                const f3x2 c = point_or_spot_x2<SPOT, LEAN>(q, pos, r.s, r.d, r.p, ok);
                direct = add3(direct, c);
            }
            redo |= ~ok;
        };
        if (!CULL) {
            for (int j = b0; j < b1; ++j) point(j);
            return;
        }
        for (int base = b0; base < b1; base += 256) {
            uint64_t ms[4];
            if (!SPOT && first != nullptr && first->valid && base == b0) {  // wave_light_terms tested these
                for (int k = 0; k < 4; ++k) ms[k] = first->m[k];
            } else {
                survivor_masks(lights, base, b1, wb, cull_enabled, ms);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint64_t m = ms[k];
                kept_total += __popcll(m);
                while (m) {
                    const int jl = base + 64 * k + __builtin_ctzll(m);
                    m &= m - 1;
                    point(jl);
                }
            }
        }
    };
    // BALANCED passes have no spot lights (host: PassArgs::balanced): nothing reads q or pos after the
    // balanced loop, so the caller can drop them across it.
    if (BALANCED)
        lighting_balanced_points<!FAITHFUL>(q, fi, pos, geo_a, geo_b, bm, *bal, bal_lights, direct, redo, bal_prof);
    else
        run_kind(std::false_type{}, pt_begin, sp_begin);
    if (!BALANCED && end > sp_begin) run_kind(std::true_type{}, sp_begin, end);
    if (FAITHFUL) {
        // The faithful loop's relative bound holds for sums of normal-range values: a nonzero sum
        // outside [2^-100, 2^100] (tiny sums, where underflowed terms -- a spot cone's pow, say -- carry
        // absolute errors of ~2^-149 that are not small relative to the sum; NaN; overflow) is redone
        // exactly. A zero sum (no light reaches the pixel: every N.L or attenuation is 0, exactly as in
        // the reference) is kept; DESIGN.md §2 states the one residue.
        const m2 in_x = eq(direct.x, 0.0f) | (ge(direct.x, 0x1p-100f) & le(direct.x, 0x1p100f));
        const m2 in_y = eq(direct.y, 0.0f) | (ge(direct.y, 0x1p-100f) & le(direct.y, 0x1p100f));
        const m2 in_z = eq(direct.z, 0.0f) | (ge(direct.z, 0x1p-100f) & le(direct.z, 0x1p100f));
        redo |= ~(in_x & in_y & in_z);
    }
    return direct;
}

// The same sum with the compiler's full IEEE sequences, for one pixel (the exact fallback and the
// PBR_FLAG_EXACT_ONLY mode). Every work-item of the block must call it (it stages lights).
template <bool CULL>
__device__ __forceinline__ void lighting_exact(const PixelInvariants& qa, const PixelInvariants& qb, f3 pa, f3 pb,
                                               bool need_a, bool need_b, const float4* __restrict__ lights,
                                               const PassArgs& ps, Lds& s, const TileBounds& tb,
                                               bool cull_enabled, f3& da, f3& db) {
    da = mk3(0.0f, 0.0f, 0.0f);
    db = mk3(0.0f, 0.0f, 0.0f);
    bool unused = true;
    for (int base = 0; base < ps.n_dir; base += kChunk) {
        const int cnt = min(kChunk, ps.n_dir - base);
        __syncthreads();
        stage_chunk<false>(lights, base, cnt, s, tb, false, true);
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float4* r = &s.light[3 * j];
            if (need_a) da = add3(da, directional_light<false>(qa, r[0], r[1], unused));
            if (need_b) db = add3(db, directional_light<false>(qb, r[0], r[1], unused));
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
            for (int j = 0; j < kept; ++j) {
                const float4* r = &s.light[3 * j];
                f3 c;
                if (need_a) {
                    const bool lit = kind == 1 ? point_or_spot_light<false, false>(qa, pa, r[0], r[1], r[2], c, unused)
                                               : point_or_spot_light<true, false>(qa, pa, r[0], r[1], r[2], c, unused);
                    if (lit) da = add3(da, c);
                }
                if (need_b) {
                    const bool lit = kind == 1 ? point_or_spot_light<false, false>(qb, pb, r[0], r[1], r[2], c, unused)
                                               : point_or_spot_light<true, false>(qb, pb, r[0], r[1], r[2], c, unused);
                    if (lit) db = add3(db, c);
                }
            }
        }
    }
}

// The exact re-pass of the pair kernel, per wave: the same per-light functions as lighting_exact (the
// compiler's IEEE sequences, reference order) with the light records read through the scalar cache instead of
// staged in LDS, so that no block barrier is needed -- a wave whose lanes need no re-pass never waits for the
// other waves of its block (the barrier cost ~4% of a wave's life in the balanced kernel). Wave-uniform.
__device__ __forceinline__ void lighting_exact_wave(const PixelInvariants& qa, const PixelInvariants& qb, f3 pa,
                                                    f3 pb, bool need_a, bool need_b, const float4* __restrict__ lights,
                                                    const PassArgs& ps, f3& da, f3& db) {
    da = mk3(0.0f, 0.0f, 0.0f);
    db = mk3(0.0f, 0.0f, 0.0f);
    bool unused = true;
    for (int j = 0; j < ps.n_dir; ++j) {
        const LightRec r = light_rec(lights, j, ps);
        if (need_a) da = add3(da, directional_light<false>(qa, r.s, r.d, unused));
        if (need_b) db = add3(db, directional_light<false>(qb, r.s, r.d, unused));
    }
    const int pt_begin = ps.n_dir, sp_begin = ps.n_dir + ps.n_point, end = sp_begin + ps.n_spot;
    for (int j = pt_begin; j < end; ++j) {
        const LightRec r = light_rec(lights, j, ps);
        const bool spot = j >= sp_begin;
        f3 c;
        if (need_a) {
            const bool lit = spot ? point_or_spot_light<true, false>(qa, pa, r.s, r.d, r.p, c, unused)
                                  : point_or_spot_light<false, false>(qa, pa, r.s, r.d, r.p, c, unused);
            if (lit) da = add3(da, c);
        }
        if (need_b) {
            const bool lit = spot ? point_or_spot_light<true, false>(qb, pb, r.s, r.d, r.p, c, unused)
                                  : point_or_spot_light<false, false>(qb, pb, r.s, r.d, r.p, c, unused);
            if (lit) db = add3(db, c);
        }
    }
}

}  // namespace

// The IEEE light sum of ONE pixel (wave-uniform `q`, `pos`) with the wave's lanes splitting the lights: lane l
// evaluates light base + l (point_or_spot_light / directional_light, the functions lighting_exact_wave calls),
// and the terms are then added in light order from +0 -- directional, point, spot, as the reference's
// ComputeLighting loops (LightingUtil.hlsl:176-199). An unlit light's term is +0, which leaves the sum as it is
// (it starts at +0 and is never -0), exactly as lighting_exact_wave's skipped addition. One evaluation of a
// light's sequence per 64 lights instead of one per light: a wave with a handful of pixels to re-pass finishes
// in a fraction of the serial loop's time (those waves were the stragglers of short launches).
__device__ __forceinline__ f3 lighting_exact_lanes(const PixelInvariants& q, f3 pos, const float4* __restrict__ lights,
                                                   const PassArgs& ps) {
    const int lane = (int)(threadIdx.x & 63);
    const int n = ps.n_dir + ps.n_point + ps.n_spot, sp_begin = ps.n_dir + ps.n_point;
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        f3 t = mk3(0.0f, 0.0f, 0.0f);
        bool unused = true;
        if (j < n) {
            const float4 r0 = lights[3 * j], r1 = lights[3 * j + 1], r2 = lights[3 * j + 2];
            if (j < ps.n_dir) {
                t = directional_light<false>(q, r0, r1, unused);
            } else {
                f3 c;
                const bool lit = j >= sp_begin ? point_or_spot_light<true, false>(q, pos, r0, r1, r2, c, unused)
                                               : point_or_spot_light<false, false>(q, pos, r0, r1, r2, c, unused);
                if (lit) t = c;
            }
        }
        const int cnt = min(64, n - base);
        for (int k = 0; k < cnt; ++k) {
            sum.x = sum.x + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.x), k));
            sum.y = sum.y + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.y), k));
            sum.z = sum.z + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t.z), k));
        }
    }
    return sum;
}

}  // namespace pbr
