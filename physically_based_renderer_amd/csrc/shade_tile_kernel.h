// shade_tile_kernel.h -- shade_tile_kernel: the pair kernel that carries every path. One workgroup per 64x8 tile
// (shade_common.h); each wave chooses its light loop (lean or general, faithful or exact, culled or uniform:
// shade_light_loops.h), and the sky pass and PBR_FLAG_EXACT_ONLY run only here. Its BAL 1 and 2 variants take the
// wave-balanced point-light lists (pbr_balanced.h); they are compiled in shade_kernels_bal.hip, BAL 0 in
// shade_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "shade_common.h"
#include "shade_wave_timeline.h"
#include "shade_light_loops.h"
#include "shade_pixel.h"

namespace pbr {

// BAL (untiled only; PassArgs::balanced): the variant whose lean waves take the wave-balanced point-light lists
// (pbr_balanced.h) -- 1: faithful passes, 2: exact passes; separate instantiations so that the other variants'
// register allocation is untouched.
template <int AMBIENT, bool F0_PLANE, bool APPLY_AO, bool CULL, int BAL = 0>
__global__ __launch_bounds__(kBlock, PBR_X2_MIN_WAVES) void shade_tile_kernel(
    GBufferArgs gb, PassArgs ps, const float4* __restrict__ lights, const float4* __restrict__ env, FrameArgs fr,
    int32_t* __restrict__ tile_kept, bool exact_only) {
    __shared__ Lds s;
    TL_BEGIN();
    PBR_PHASE("entry");
#if PBR_BAL_PROFILE
    const long long t_entry = (long long)__builtin_amdgcn_s_memtime();
    unsigned long long* bal_prof = s.prof[__builtin_amdgcn_readfirstlane(threadIdx.x) >> 6];
    if ((threadIdx.x & 63) < 16) bal_prof[threadIdx.x & 63] = 0;
#endif
    load_libm_tables<AMBIENT == kAmbientIblDiffuse, kBlock>();  // powf (+ atanf with IBL) tables -> LDS
    if constexpr (BAL != 0)
        stage_balanced_lights<kBlock>(lights, ps.n_dir, ps.n_dir + ps.n_point, s.bal_light, BAL == 2 ? 4.0f : 1.0f);
    __syncthreads();
    PBR_PHASE("load_window");

    // wave_id: the wave's two rows of the tile (wave-uniform, SGPR); wslot: its exchange region in this workgroup (a
    // name of its own: folded into wave_id, the exact balanced kernels schedule one instruction differently).
    const int wave_id = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
    const int wslot = wave_id;
    const int tile_y = (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    const int xa = blockIdx.x * kTileW + 2 * (tid & 31);
    const int y = tile_y * kTileH + (tid >> 5);
    const bool va = (xa < gb.width) && (y < gb.height);
    const bool vb = (xa + 1 < gb.width) && (y < gb.height);
    const int64_t row = (int64_t)y * gb.row_stride;
    // Geometry (PS) or background (sky pass) per pixel; background pixels take no part in the tile
    // bounds, the exact re-pass or the lighting (a block without geometry skips it).
    const bool ga = va && is_geometry(fr, xa, y), gb_ = vb && is_geometry(fr, xa + 1, y);
    const bool wave_geometry = lanes(ga || gb_) != 0;  // waves wholly outside the frame skip lighting

    PairIn p = load_pair<F0_PLANE, APPLY_AO>(gb, ps, va ? row + xa : 0, vb ? row + xa + 1 : 0,
                                             vb && gb.pairs_aligned);
    const f3 pa = lane(p.pos, 0), pb = lane(p.pos, 1);

    const bool ok_a = !exact_only && ps.eye_ok && fast_window_ok(pa, lane(p.n, 0), lane(p.albedo, 0), lane(p.f0, 0),
                                                    p.metallic.x, p.roughness.x);
    const bool ok_b = !exact_only && ps.eye_ok && fast_window_ok(pb, lane(p.n, 1), lane(p.albedo, 1), lane(p.f0, 1),
                                                    p.metallic.y, p.roughness.y);
    const m2 fast2 = mask2(ok_a, ok_b);
    TL_LOADED();

    // The pair's invariants. Balanced variants form them on each path that needs them (their balanced paths build
    // their own after pass 1, so computing them here left one dead pair_invariants on the common path); the
    // uniform and culled variants form them here (formed per path, the max-ILP build spilled 20-36 B/lane).
    PixelInvariants2 q2;
    if constexpr (BAL == 0) q2 = pair_invariants(p, ps, fast2);
    auto form_q2 = [&]() {
        if constexpr (BAL != 0) q2 = pair_invariants(p, ps, fast2);
    };

    // The wave's world-space box (its 64x2 pixels; background pixels excluded): wave64 butterflies,
    // then scalar registers. Non-finite positions disable culling for the wave (the reference's
    // NaN/inf behaviour at LightingUtil.hlsl:131 is then reproduced light by light).
    TileBounds wb{};
    bool cull_enabled = false;
    if (CULL) {
        const bool finite = (!ga || (isfinite(pa.x) && isfinite(pa.y) && isfinite(pa.z))) &&
                            (!gb_ || (isfinite(pb.x) && isfinite(pb.y) && isfinite(pb.z)));
        const float big = 3.0e38f;
        wb.mn[0] = uniform_f(wave_min(fminf(ga ? pa.x : big, gb_ ? pb.x : big)));
        wb.mn[1] = uniform_f(wave_min(fminf(ga ? pa.y : big, gb_ ? pb.y : big)));
        wb.mn[2] = uniform_f(wave_min(fminf(ga ? pa.z : big, gb_ ? pb.z : big)));
        wb.mx[0] = uniform_f(wave_max(fmaxf(ga ? pa.x : -big, gb_ ? pb.x : -big)));
        wb.mx[1] = uniform_f(wave_max(fmaxf(ga ? pa.y : -big, gb_ ? pb.y : -big)));
        wb.mx[2] = uniform_f(wave_max(fmaxf(ga ? pa.z : -big, gb_ ? pb.z : -big)));
        cull_enabled = lanes(!finite) == 0;
    }

    // ComputeLighting (LightingUtil.hlsl:170-200) on the packed fast path. From here on the pair
    // lives only in packed form (q2, pos2); the scalar views are rebuilt from it afterwards so the
    // loop does not carry two copies of the invariants.
    int kept_total = 0;
    int bal_items = -1;  // wave-uniform: the balanced pass's live point-light items (statistics), -1 = not run
    m2 redo = m2{0, 0};
    f3x2 pos2 = p.pos;
    f3x2 d2 = splat3(0.0f, 0.0f, 0.0f);
    bool faithful_wave = false;  // wave-uniform: the faithful loop ran, so the finish may be faithful too
    TL_RT(3);
    // The balanced variants: one vote of the workgroup, in which every wave takes part whatever path it chooses below.
    // A wave that runs this instantiation's balanced pass votes for ranking with the whole workgroup and meets the
    // others at the vote's barrier after its pass 1 (lighting_balanced_points); every other wave -- outside the frame,
    // background only, on another light loop, an exact_only pass -- votes no and takes the barrier at once. Where all
    // four vote yes they rank and exchange their 512 pixels together (pbr_balanced.h), and that unanimity is what makes
    // block barriers legal inside a path the waves otherwise choose one by one; else each balanced wave ranks its own
    // 128. kBalRankPerWave in ps.balanced (a development switch) makes every vote a no.
    auto vote = [&](bool yes) {
        if ((tid & 63) == 0) s.bal[wslot].vote = yes;
    };
    auto vote_no = [&]() {
        if constexpr (BAL != 0) {
            vote(false);
            __syncthreads();
        }
    };
    if (wave_geometry) {  // wave-uniform
        // Wave-uniform choice of the light loop.
        const v2 nn = dot3(p.n, p.n);
        const bool lean_lane = ok_a && ok_b && nn.x <= 1.0f + 0x1p-20f && nn.y <= 1.0f + 0x1p-20f &&
                               f0_nonzero(lane(p.f0, 0)) && f0_nonzero(lane(p.f0, 1));  // make_invariants' f0_nonzero
        // PBR_FLAG_FAITHFUL (host-validated: strengths, ambient and env texels >= 0): in a wave inside the
        // fast window whose albedo is >= 0 and F0 in [0, 1] every light's contribution is >= 0, which bounds
        // the error of the faithful divisions in the sum (brdf_faithful_x2). ps.faithful == 2: a culled pass
        // with more lights than the bound's 64 summed terms, counted per wave here.
        const bool faithful_lane =
            ps.faithful && ok_a && ok_b && p.albedo.x.x >= 0.0f && p.albedo.y.x >= 0.0f && p.albedo.z.x >= 0.0f &&
            p.albedo.x.y >= 0.0f && p.albedo.y.y >= 0.0f && p.albedo.z.y >= 0.0f && p.f0.x.x <= 1.0f &&
            p.f0.y.x <= 1.0f && p.f0.z.x <= 1.0f && p.f0.x.y <= 1.0f && p.f0.y.y <= 1.0f && p.f0.z.y <= 1.0f &&
            p.f0.x.x >= 0.0f && p.f0.y.x >= 0.0f && p.f0.z.x >= 0.0f && p.f0.x.y >= 0.0f && p.f0.y.y >= 0.0f &&
            p.f0.z.y >= 0.0f;
        // BAL == 2 kernels shade exact passes only (host: PassArgs::balanced): no faithful code is compiled in.
        faithful_wave = BAL != 2 && ps.faithful && lanes(!faithful_lane) == 0;
        if (CULL && faithful_wave && ps.faithful == 2)
            faithful_wave = wave_light_terms(lights, ps, wb, cull_enabled) <= kFaithfulMaxTerms;
        const bool lean_wave = lanes(!lean_lane) == 0;
        // Untiled faithful waves read rescaled invariants (exact both ways, faithful_scale).
        if (faithful_wave && lean_wave) {
            if constexpr (BAL == 1 && !CULL) {
#if PBR_BAL_PROFILE
                BAL_PROF_ADD(7, (long long)__builtin_amdgcn_s_memtime() - t_entry);
                unsigned long long* prof = s.prof[wslot];
#else
                unsigned long long* prof = nullptr;
#endif
                // Pass 1 on the raw pair; then the scaled invariants for the loop, rebuilt from the raw pair (the
                // q2 above is not used on this path, so it is not live across pass 1); after the loop the
                // unscaled ones once more for the finish. launder() keeps the compiler from merging the
                // rebuilds with the computation above (which would keep q2 live across the loop: it spilled).
                PBR_PHASE("pass1");
                vote(!(ps.balanced & kBalRankPerWave));
                const BalMasks bm = balanced_pass1<false>(p.pos, p.n, ga, gb_, ps.n_point, kBalDistLoFaithful, s.bal[wslot],
                                                   s.bal_light, prof);
                bal_items = wave_live_items(bm);
                PBR_PHASE("invariants");
                launder(p);
                q2 = pair_invariants(p, ps, fast2);
                faithful_scale(q2);
                d2 = lighting_fast<false, true, true, true>(q2, p.pos, fast2, lights, ps, wb, cull_enabled, redo,
                                                            kept_total, &s.bal[wslot], s.bal_light, ga, gb_, bm,
                                                            prof);
#if PBR_BAL_PROFILE
                const long long t_l1 = (long long)__builtin_amdgcn_s_memtime();
#endif
                PBR_PHASE("invariants2");
                launder(p);
                q2 = pair_finish_invariants(p, ps, fast2);  // the rare exact re-pass reads its pixels again
                pos2 = p.pos;
#if PBR_BAL_PROFILE
                const v2 dep = dot3(q2.n, q2.v);
                if (dep.x == 12345.0f) pos2.x.x = 0.5f;
                BAL_PROF_ADD(8, (long long)__builtin_amdgcn_s_memtime() - t_l1);
#endif
            } else {
                vote_no();
                form_q2();
                if (!CULL) faithful_scale(q2);
#if PBR_BAL_PROFILE
                const long long t_u0 = (long long)__builtin_amdgcn_s_memtime();
                BAL_PROF_ADD(11, t_u0 - t_entry);
                BAL_PROF_ADD(13, 1);
#endif
                d2 = lighting_fast<CULL, true, true>(q2, pos2, fast2, lights, ps, wb, cull_enabled, redo, kept_total);
                if (!CULL) faithful_unscale(q2);
#if PBR_BAL_PROFILE
                const v2 dep = d2.x + d2.y;
                if (dep.x == 12345.0f) pos2.x.x = 0.5f;
                BAL_PROF_ADD(12, (long long)__builtin_amdgcn_s_memtime() - t_u0);
#endif
            }
        } else if (faithful_wave) {
            PBR_COLD("faithful_nonlean");
            vote_no();
            form_q2();
            if (!CULL) faithful_scale(q2);
            d2 = lighting_fast<CULL, false, true>(q2, pos2, fast2, lights, ps, wb, cull_enabled, redo, kept_total);
            if (!CULL) faithful_unscale(q2);
        } else if (lean_wave) {
            PBR_PHASE("xpass1");  // the exact balanced kernel's path (the faithful census stops here)
            if constexpr (BAL == 2 && !CULL) {
#if PBR_BAL_PROFILE
                unsigned long long* prof = s.prof[wslot];
#else
                unsigned long long* prof = nullptr;
#endif
                // Nothing of the raw pair is carried through the loop: it is read from the G-buffer again
                // afterwards (44 B/px). Carrying it spilled (~250 B/px of scratch traffic): the exact loop's
                // temporaries leave no room for it. The offsets are re-derived from the hardware ids
                // (lane_id_fresh) and the memory clobber keeps the compiler from reusing the first load.
                // (Reading it once more after pass 1 too, so that only position and normal live through
                // pass 1, removed the remaining scratch of this path but measured the same.)
                auto reload = [&]() {
                    asm volatile("" ::: "memory");
                    const int rl = lane_id_fresh();
                    const int rx = blockIdx.x * kTileW + 2 * (rl & 31);
                    const int ry = tile_y * kTileH + 2 * wave_id + (rl >> 5);
                    const int64_t rrow = (int64_t)ry * gb.row_stride + rx;
                    p = load_pair<F0_PLANE, APPLY_AO>(gb, ps, va ? rrow : 0, vb ? rrow + 1 : 0,
                                                      vb && gb.pairs_aligned);
                };
                vote(!(ps.balanced & kBalRankPerWave));
                const BalMasks bm = balanced_pass1<true>(p.pos, p.n, ga, gb_, ps.n_point, kBalDistLoExact, s.bal[wslot],
                                                   s.bal_light, prof);
                bal_items = wave_live_items(bm);
                PBR_PHASE("xinvariants");
                q2 = pair_invariants(p, ps, fast2);
                d2 = lighting_fast<false, true, false, true>(q2, p.pos, fast2, lights, ps, wb, cull_enabled, redo,
                                                             kept_total, &s.bal[wslot], s.bal_light, ga, gb_, bm,
                                                             prof);
                PBR_PHASE("xinvariants2");
                reload();
                q2 = pair_invariants(p, ps, fast2);  // the full set: the finish-only one measured slower here (SGPRs)
                pos2 = p.pos;
            } else {
                vote_no();
                form_q2();
                d2 = lighting_fast<CULL, true>(q2, pos2, fast2, lights, ps, wb, cull_enabled, redo, kept_total);
            }
        } else {
            PBR_COLD("general");
            vote_no();
            form_q2();
            d2 = lighting_fast<CULL, false>(q2, pos2, fast2, lights, ps, wb, cull_enabled, redo, kept_total);
        }
    } else {
        PBR_COLD("background");
        vote_no();
        form_q2();  // background only: the sky pass reads N
    }
    TL_RT(4);
    const PixelInvariants ua = unpack_invariants(q2, 0), ub = unpack_invariants(q2, 1);
    f3 da = lane(d2, 0), db = lane(d2, 1);
    const bool need_a = ga && on(redo.x), need_b = gb_ && on(redo.y);
    // Statistics, one record per wave (kStatsPerBlock ints at slot tile * 4 + wave): culling survivors and
    // whether the wave has geometry (culled passes), the pixels it sends to the exact path, and the work the
    // light loops executed for its geometry pixels: light terms evaluated (every light of the pass in the
    // uniform loop, the survivors of the wave's box under culling, the live items of the balanced lists) and
    // the balanced pass-1 back-face tests.
    PBR_PHASE("stats_repass");
    const int n_exact = __popcll(lanes(need_a)) + __popcll(lanes(need_b));
    const int geo_px = __popcll(lanes(ga)) + __popcll(lanes(gb_));
    if ((tid & 63) == 0 && tile_kept != nullptr) {
        const int64_t slot = ((int64_t)tile_y * gridDim.x + blockIdx.x) * (kBlock / 64) + wave_id;
        const int n_ps = CULL ? kept_total : ps.n_point + ps.n_spot;
        const int terms = !wave_geometry ? 0 : bal_items >= 0 ? bal_items + ps.n_dir * geo_px : (ps.n_dir + n_ps) * geo_px;
        int32_t* st = tile_kept + kStatsPerBlock * slot;
        st[kStatCullKept] = CULL && wave_geometry ? kept_total : 0;
        st[kStatCullTiles] = CULL && wave_geometry ? 1 : 0;
        st[kStatExactPixels] = n_exact;
        st[kStatLightTerms] = terms;
        st[kStatGeometryPixels] = geo_px;
        st[kStatBackfaceTests] = wave_geometry && bal_items >= 0 ? ps.n_point * geo_px : 0;
    }
#if PBR_BAL_PROFILE
    const long long t_b0 = (long long)__builtin_amdgcn_s_memtime();
#endif
    // The balanced variants re-pass their pixels after the stores (repass_exact, as shade_lean_kernel): up to
    // kLanesRepassMax pixels one at a time with the lanes splitting the lights, instead of every light for the
    // whole wave here (~50 us for one pixel, which made the few waves that have one the launch's last).
    if (BAL == 0 && n_exact != 0) {  // wave-uniform: rare (edge inputs, EXACT_ONLY)
        PBR_COLD("exact_repass");
        f3 ea, eb;
        lighting_exact_wave(ua, ub, lane(pos2, 0), lane(pos2, 1), need_a, need_b, lights, ps, ea, eb);
        if (need_a) da = ea;
        if (need_b) db = eb;
    }

#if PBR_BAL_PROFILE
    {
        const long long t_b1 = (long long)__builtin_amdgcn_s_memtime();
        BAL_PROF_ADD(BAL ? 6 : 15, t_b1 - t_entry);
        BAL_PROF_ADD(BAL ? 9 : 14, t_b1 - t_b0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int l = threadIdx.x & 63;
        const int64_t wv = ((int64_t)tile_y * gridDim.x + blockIdx.x) * (kBlock / 64) + wave_id;
        if (l < 16 && g_bal_prof_buf != nullptr && wv < (int64_t)(1 << 18)) g_bal_prof_buf[wv * 16 + l] += bal_prof[l];
    }
#endif
    // The output offset re-derived from the hardware ids (lane_id_fresh): same pixel as xa, y above.
    PBR_PHASE("finish_setup");
    const int ln = lane_id_fresh();
    const int sx = blockIdx.x * kTileW + 2 * (ln & 31);
    const int64_t orow = (int64_t)(tile_y * kTileH + 2 * wave_id + (ln >> 5)) * fr.out_stride + sx;
    // PBR_FLAG_APPLY_AO: the AO pair is read only now, for the finish (Default.hlsl:150 ambient * AO): a value
    // loaded at entry would be live across the light loops (it was the one spilled value of the AO kernels).
    float ao_a = 1.0f, ao_b = 1.0f;
    if (APPLY_AO) {
        const int64_t arow = (int64_t)(tile_y * kTileH + 2 * wave_id + (ln >> 5)) * gb.row_stride + sx;
        if (vb && gb.pairs_aligned) {
            const float2 t = *reinterpret_cast<const float2*>(
                gb.plane[11] + PBR_BOUNDS_PIXEL(arow, gb.width, gb.height, gb.row_stride, 2, kBoundsGBuffer));
            ao_a = t.x;
            ao_b = t.y;
        } else {
            if (va) ao_a = gb.plane[11][PBR_BOUNDS_PIXEL(arow, gb.width, gb.height, gb.row_stride, 1, kBoundsGBuffer)];
            if (vb)
                ao_b = gb.plane[11][PBR_BOUNDS_PIXEL(arow + 1, gb.width, gb.height, gb.row_stride, 1, kBoundsGBuffer)];
        }
    }
    float4 ca = make_float4(0.0f, 0.0f, 0.0f, 0.0f), cb = ca;
    const bool live_a = ga && !(BAL != 0 && need_a), live_b = gb_ && !(BAL != 0 && need_b);
    if (lanes(live_a || live_b) != 0)  // wave-uniform
        finish_pair<AMBIENT, APPLY_AO>(q2, ua, ub, ao_a, ao_b, da, db, ps, env, ok_a, ok_b, faithful_wave, live_a,
                                       live_b, ca, cb);
    PBR_PHASE("store");
    if (va && !ga) ca = sky_pixel(ua.n, ps, fr.sky, !exact_only);
    if (vb && !gb_) cb = sky_pixel(ub.n, ps, fr.sky, !exact_only);
    bool keep_a, keep_b;
    alpha_keep_pair(gb, (int64_t)(tile_y * kTileH + 2 * wave_id + (ln >> 5)) * gb.row_stride + sx, ga, gb_, ca,
                    cb, keep_a, keep_b);
    if (va && keep_a && !(BAL != 0 && need_a)) store_pixel(fr, orow, ca);
    if (vb && keep_b && !(BAL != 0 && need_b)) store_pixel(fr, orow + 1, cb);
    if (BAL != 0 && n_exact != 0)  // wave-uniform
        repass_exact<AMBIENT, F0_PLANE, APPLY_AO>(gb, ps, lights, env, fr, blockIdx.x, tile_y, wave_id, need_a, need_b,
                                                  n_exact, faithful_wave);
    TL_END(((long long)tile_y * gridDim.x + blockIdx.x) * (kBlock / 64) + wave_id);
}

}  // namespace pbr
