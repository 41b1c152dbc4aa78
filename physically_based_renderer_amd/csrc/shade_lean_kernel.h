// shade_lean_kernel.h -- the lean pair kernel.
//
// shade_tile_kernel's register allocation is the maximum over every path it carries, and its exact re-pass runs
// with the fast path's state (invariants, positions, sums) still live around it. shade_lean_kernel is the same
// per-wave choice of fast loops for uniform-loop passes (no balanced lists) without a sky pass, but it finishes
// and stores every pixel the fast loop settled first, and only then re-passes the pixels the loop sent to the
// exact path, one at a time, reading each back from the G-buffer and evaluating it with the IEEE sequences
// (shade_pixel_exact; the finish of its wave: faithful in a faithful wave). Nothing of the fast path is live
// there, so the rare path does not raise the register peak of the loops, and the faithful-only instantiation
// (FAITHFUL: the pass has PBR_FLAG_FAITHFUL) carries no faithful code in the exact-mode one. Frames and pass
// statistics are bit-identical to shade_tile_kernel's (tests/test_gpu_lean.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "shade_common.h"
#include "shade_wave_timeline.h"
#include "shade_light_loops.h"
#include "shade_pixel.h"

namespace pbr {

// One wave's 64x2 pixels: wave wave_id (tile rows 2 wave_id, 2 wave_id + 1) of tile (tile_x, tile_y), statistics
// slot wave_global. The caller has staged the powf tables.
template <int AMBIENT, bool F0_PLANE, bool APPLY_AO, bool CULL, bool FAITHFUL>
__device__ __forceinline__ void lean_wave(const GBufferArgs& gb, const PassArgs& ps, const float4* __restrict__ lights,
                                          const float4* __restrict__ env, const FrameArgs& fr,
                                          int32_t* __restrict__ tile_kept, int tile_x, int tile_y, int wave_id,
                                          int64_t wave_global) {
    TL_BEGIN();
    const int tid = threadIdx.x;
    const int xa = tile_x * kTileW + 2 * (tid & 31);
    const int y = tile_y * kTileH + 2 * wave_id + (tid >> 5);
    const bool va = (xa < gb.width) && (y < gb.height);
    const bool vb = (xa + 1 < gb.width) && (y < gb.height);
    const int geo_px = __popcll(lanes(va)) + __popcll(lanes(vb));
    if (geo_px == 0) {  // wholly outside the frame: nothing to shade, an empty statistics record
        if ((tid & 63) == 0 && tile_kept != nullptr) {
            int32_t* st = tile_kept + kStatsPerBlock * wave_global;
            for (int i = 0; i < kStatsPerBlock; ++i) st[i] = 0;
        }
        return;
    }
    const int64_t row = (int64_t)y * gb.row_stride;
    constexpr bool kPark = lean_min_waves<AMBIENT, CULL, FAITHFUL>() >= 5;
    __shared__ v2 s_park[4][64];   // five-wave kernels' faithful waves: albedo, 1 - metallic across the light loop
    bool need_a, need_b;           // pixels for the IEEE path (the exact re-pass)
    bool faithful_wave = false;    // wave-uniform
    int kept_total = 0;
    {
        // Culled passes without spot lights: the first 256 point lights' positions (lane j: light n_dir + 64 k + j)
        // are loaded before the pair, so the culling box and the survivor tests below overlap the G-buffer loads'
        // latency instead of following it; the survivor masks then serve the term count and the walk. (Issuing them
        // between the position planes and the other planes measured 3.5% slower on config 4: the per-lane choice of
        // load form makes the later planes wait for the light loads.)
        float4 lp[4];
        const bool early = CULL && ps.n_spot == 0 && ps.n_point > 0;  // wave-uniform
        if (CULL && early) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = ps.n_dir + 64 * k + tid;
                lp[k] = j < ps.n_dir + ps.n_point ? lights[3 * PBR_BOUNDS(j, ps.n_dir + ps.n_point, kBoundsLight) + 2]
                                                  : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        PairIn p = load_pair<F0_PLANE, APPLY_AO>(gb, ps, va ? row + xa : 0, vb ? row + xa + 1 : 0,
                                                 vb && gb.pairs_aligned);
        TileBounds wb{};
        bool cull_enabled = false;
        FirstSurvivors first;  // the first survivor masks, for the faithful term count and the culled walk
        if (CULL) {  // the wave's box, as in shade_tile_kernel (every pixel is geometry: no sky pass)
            const f3 pa = lane(p.pos, 0), pb = lane(p.pos, 1);
            const bool finite = (!va || (isfinite(pa.x) && isfinite(pa.y) && isfinite(pa.z))) &&
                                (!vb || (isfinite(pb.x) && isfinite(pb.y) && isfinite(pb.z)));
            const float big = 3.0e38f;
            wb.mn[0] = uniform_f(wave_min(fminf(va ? pa.x : big, vb ? pb.x : big)));
            wb.mn[1] = uniform_f(wave_min(fminf(va ? pa.y : big, vb ? pb.y : big)));
            wb.mn[2] = uniform_f(wave_min(fminf(va ? pa.z : big, vb ? pb.z : big)));
            wb.mx[0] = uniform_f(wave_max(fmaxf(va ? pa.x : -big, vb ? pb.x : -big)));
            wb.mx[1] = uniform_f(wave_max(fmaxf(va ? pa.y : -big, vb ? pb.y : -big)));
            wb.mx[2] = uniform_f(wave_max(fmaxf(va ? pa.z : -big, vb ? pb.z : -big)));
            cull_enabled = lanes(!finite) == 0;
            if (early && cull_enabled) {  // survivor_masks' tests on the preloaded positions
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    first.m[k] = lanes(ps.n_dir + 64 * k + tid < ps.n_dir + ps.n_point && light_survives(lp[k], wb));
                first.valid = true;
            }
        }
        // shade_tile_kernel's per-wave choice of the light loop (BAL 0, every pixel geometry), unchanged.
        const bool ok_a = ps.eye_ok && fast_window_ok(lane(p.pos, 0), lane(p.n, 0), lane(p.albedo, 0),
                                                      lane(p.f0, 0), p.metallic.x, p.roughness.x);
        const bool ok_b = ps.eye_ok && fast_window_ok(lane(p.pos, 1), lane(p.n, 1), lane(p.albedo, 1),
                                                      lane(p.f0, 1), p.metallic.y, p.roughness.y);
        const m2 fast2 = mask2(ok_a, ok_b);
        TL_LOADED();
        PixelInvariants2 q2 = pair_invariants(p, ps, fast2);
        const v2 nn = dot3(p.n, p.n);
        const bool lean_lane = ok_a && ok_b && nn.x <= 1.0f + 0x1p-20f && nn.y <= 1.0f + 0x1p-20f &&
                               on(q2.f0_nonzero.x) && on(q2.f0_nonzero.y);
        if (FAITHFUL) {
            const bool faithful_lane =
                ok_a && ok_b && p.albedo.x.x >= 0.0f && p.albedo.y.x >= 0.0f && p.albedo.z.x >= 0.0f &&
                p.albedo.x.y >= 0.0f && p.albedo.y.y >= 0.0f && p.albedo.z.y >= 0.0f && p.f0.x.x <= 1.0f &&
                p.f0.y.x <= 1.0f && p.f0.z.x <= 1.0f && p.f0.x.y <= 1.0f && p.f0.y.y <= 1.0f && p.f0.z.y <= 1.0f &&
                p.f0.x.x >= 0.0f && p.f0.y.x >= 0.0f && p.f0.z.x >= 0.0f && p.f0.x.y >= 0.0f && p.f0.y.y >= 0.0f &&
                p.f0.z.y >= 0.0f;
            faithful_wave = lanes(!faithful_lane) == 0;
            if (CULL && faithful_wave && ps.faithful == 2)
                faithful_wave = wave_light_terms(lights, ps, wb, cull_enabled, &first) <= kFaithfulMaxTerms;
        }
        const bool lean_wave = lanes(!lean_lane) == 0;
        TL_RT(3);
        m2 redo = m2{0, 0};
        f3x2 d2;
        if (faithful_wave) {
            if (!CULL) faithful_scale(q2);
            // Five-wave kernels: albedo and 1 - metallic feed the faithful loop only through make_faithful's hoisted
            // products, but the finish needs them; parked in LDS across the loop (the memory clobber keeps the
            // compiler from forwarding the stored values), they hold no VGPRs there: at the 96-VGPR budget of five
            // waves per SIMD the loop then runs without scratch.
            if constexpr (kPark) {
                const int l = (int)(threadIdx.x & 63);
                s_park[0][l] = q2.albedo.x;
                s_park[1][l] = q2.albedo.y;
                s_park[2][l] = q2.albedo.z;
                s_park[3][l] = q2.one_minus_metal;
                asm volatile("" ::: "memory");
            }
            if (lean_wave)
                d2 = lighting_fast<CULL, true, true>(q2, p.pos, fast2, lights, ps, wb, cull_enabled, redo, kept_total,
                                                     nullptr, nullptr, false, false, BalMasks{}, nullptr, &first);
            else
                d2 = lighting_fast<CULL, false, true>(q2, p.pos, fast2, lights, ps, wb, cull_enabled, redo, kept_total,
                                                      nullptr, nullptr, false, false, BalMasks{}, nullptr, &first);
            if constexpr (kPark) {
                asm volatile("" ::: "memory");
                const int l = lane_id_fresh();
                q2.albedo = f3x2{s_park[0][l], s_park[1][l], s_park[2][l]};
                q2.one_minus_metal = s_park[3][l];
            }
            if (!CULL) faithful_unscale(q2);
        } else if (lean_wave) {
            d2 = lighting_fast<CULL, true>(q2, p.pos, fast2, lights, ps, wb, cull_enabled, redo, kept_total,
                                           nullptr, nullptr, false, false, BalMasks{}, nullptr, &first);
        } else {
            d2 = lighting_fast<CULL, false>(q2, p.pos, fast2, lights, ps, wb, cull_enabled, redo, kept_total,
                                            nullptr, nullptr, false, false, BalMasks{}, nullptr, &first);
        }
        TL_RT(4);
        {
            need_a = va && on(redo.x);
            need_b = vb && on(redo.y);
            // Finish and store every pixel the fast loop settled.
            const PixelInvariants ua = unpack_invariants(q2, 0), ub = unpack_invariants(q2, 1);
            const int ln = lane_id_fresh();
            const int sx = tile_x * kTileW + 2 * (ln & 31);
            const int64_t orow = (int64_t)(tile_y * kTileH + 2 * wave_id + (ln >> 5)) * fr.out_stride + sx;
            float ao_a = 1.0f, ao_b = 1.0f;
            if (APPLY_AO) {
                const int64_t arow = (int64_t)(tile_y * kTileH + 2 * wave_id + (ln >> 5)) * gb.row_stride + sx;
                if (vb && gb.pairs_aligned) {
                    const float2 t = *reinterpret_cast<const float2*>(
                        gb.plane[11] + PBR_BOUNDS_PIXEL(arow, gb.width, gb.height, gb.row_stride, 2, kBoundsGBuffer));
                    ao_a = t.x;
                    ao_b = t.y;
                } else {
                    if (va)
                        ao_a = gb.plane[11][PBR_BOUNDS_PIXEL(arow, gb.width, gb.height, gb.row_stride, 1,
                                                             kBoundsGBuffer)];
                    if (vb)
                        ao_b = gb.plane[11][PBR_BOUNDS_PIXEL(arow + 1, gb.width, gb.height, gb.row_stride, 1,
                                                             kBoundsGBuffer)];
                }
            }
            float4 ca = make_float4(0.0f, 0.0f, 0.0f, 0.0f), cb = ca;
            finish_pair<AMBIENT, APPLY_AO>(q2, ua, ub, ao_a, ao_b, lane(d2, 0), lane(d2, 1), ps, env, ok_a, ok_b,
                                           faithful_wave, va && !need_a, vb && !need_b, ca, cb);
            bool keep_a, keep_b;
            alpha_keep_pair(gb, (int64_t)(tile_y * kTileH + 2 * wave_id + (ln >> 5)) * gb.row_stride + sx,
                            va && !need_a, vb && !need_b, ca, cb, keep_a, keep_b);
            if (va && !need_a && keep_a) store_pixel(fr, orow, ca);
            if (vb && !need_b && keep_b) store_pixel(fr, orow + 1, cb);
        }
    }
    const int n_exact = __popcll(lanes(need_a)) + __popcll(lanes(need_b));
    if ((tid & 63) == 0 && tile_kept != nullptr) {
        const bool culled = CULL;
        const int n_ps = culled ? kept_total : ps.n_point + ps.n_spot;
        int32_t* st = tile_kept + kStatsPerBlock * wave_global;
        st[kStatCullKept] = culled ? kept_total : 0;
        st[kStatCullTiles] = culled ? 1 : 0;
        st[kStatExactPixels] = n_exact;
        st[kStatLightTerms] = (ps.n_dir + n_ps) * geo_px;
        st[kStatGeometryPixels] = geo_px;
        st[kStatBackfaceTests] = 0;
    }
    if (n_exact != 0)  // wave-uniform, rare: the IEEE path
        repass_exact<AMBIENT, F0_PLANE, APPLY_AO>(gb, ps, lights, env, fr, tile_x, tile_y, wave_id, need_a, need_b,
                                                  n_exact, faithful_wave);
    TL_FLAGS((n_exact != 0 ? 1 : 0) | (FAITHFUL && !faithful_wave ? 2 : 0));
    TL_END(wave_global);
}

// One wave per workgroup (blockIdx.y = 4 * tile row + wave): a wave's slot on its SIMD is refilled as soon as it
// ends (with 4-wave workgroups a new workgroup waited for four free slots on the CU). Tried and dropped: a
// persistent grid of 3 or 4 waves per SIMD walking the waves (same-box A/B config 2 0.058 -> 0.090 ms: each wave
// then waits for its own G-buffer loads, which the independent waves overlap).
template <int AMBIENT, bool F0_PLANE, bool APPLY_AO, bool CULL, bool FAITHFUL>
__global__ __launch_bounds__(64, (lean_min_waves<AMBIENT, CULL, FAITHFUL>())) void shade_lean_kernel(GBufferArgs gb, PassArgs ps,
                                                            const float4* __restrict__ lights,
                                                            const float4* __restrict__ env, FrameArgs fr,
                                                            int32_t* __restrict__ tile_kept) {
    // powf tables -> LDS: the exact finish's gamma, spot cones, the faithful gamma's edges (+ atanf rows with IBL)
    load_libm_tables<AMBIENT == kAmbientIblDiffuse, 64>();
    __syncthreads();
    lean_wave<AMBIENT, F0_PLANE, APPLY_AO, CULL, FAITHFUL>(gb, ps, lights, env, fr, tile_kept, blockIdx.x,
                                                           blockIdx.y >> 2, blockIdx.y & 3,
                                                           ((int64_t)(blockIdx.y >> 2) * gridDim.x + blockIdx.x) *
                                                                   (kBlock / 64) + (blockIdx.y & 3));
}

}  // namespace pbr
