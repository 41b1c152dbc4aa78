// tests/libm_x2_paths.cpp -- host program of tests/test_libm_x2_paths.py: the main and patch parts of the pair forms
// (csrc/libm_f32_x2.h, LIBM_F32_HOST) against the scalar restatement pbr_atan2f / pbr_asinf (csrc/libm_f32.h), bit for
// bit, on directed inputs and a seeded random sample. For every input it also evaluates the MAIN path alone and
// classifies the element as the kernel does (odd -> special or rare), and checks
//   * soundness: an element that is not odd has main == scalar;
//   * the flags' definitions: special is the window predicate; rare is odd and not special;
//   * the composed form (main + patch) == scalar on every element that is not special;
//   * the keyed 81-row table reads the same row as the five-row index, and gives the same result;
//   * that the flags matter: per rare class it counts the inputs on which the main path alone differs from the
//     scalar function (printed; the Python test requires every class to be hit: a `rare` that is never set, or a
//     patch that is never needed, does not pass).
// Prints "name value" lines; exit status 0 iff no mismatch.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#define LIBM_F32_HOST 1
#include "libm_f32_x2.h"

static const pbr_atan_seg kTab5[5] = PBR_ATAN_SEG_TABLE_INIT;
static const pbr_atan_seg kTabKeyed[PBR_ATAN_KEYS] = PBR_ATAN_SEG_KEYED_INIT;

static inline uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float bitsf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline int same(float a, float b) { return fbits(a) == fbits(b) || (a != a && b != b); }

enum { kZeroY, kZeroX, kGapBig, kGapNeg, kHuge, kAsinOne, kClasses };
static const char* kClassName[kClasses] = {"zero_y", "zero_x", "gap_big", "gap_neg", "quotient_huge", "asin_one"};

static uint64_t g_n_atan2, g_n_asin, g_bad_sound, g_bad_flags, g_bad_composed, g_bad_keyed, g_rare, g_special;
static uint64_t g_class_seen[kClasses], g_class_main_differs[kClasses];

static void check_atan2_pair(float y0, float x0, float y1, float x1) {
    const pbr_lv2 y = {y0, y1}, x = {x0, x1};
    int odd[2], oddk[2], special[2], special_c[2];
    pbr_lv2 q, qk;
    const pbr_lv2 z = pbr_atan2f_x2_head(y, x, odd, &q, kTab5, 0);
    const pbr_lv2 zk = pbr_atan2f_x2_head(y, x, oddk, &qk, kTabKeyed, 1);
    const pbr_lv2 main_r = pbr_atan2f_x2_tail(y, x, z);
    const pbr_lv2 patched = pbr_atan2f_x2_tail_patch(y, x, q, z);
    pbr_atan2f_x2_special(y, x, special);
    const pbr_lv2 composed = pbr_atan2f_x2(y, x, special_c, kTab5);
    for (int e = 0; e < 2; ++e) {
        const float ye = e ? y1 : y0, xe = e ? x1 : x0;
        const float want = pbr_atan2f(ye, xe);
        const float ya = fabsf(ye), xa = fabsf(xe);
        const int need_special = !((ya == 0.0f || (ya >= 0x1p-40f && ya <= 0x1p40f)) &&
                                   (xa == 0.0f || (xa >= 0x1p-40f && xa <= 0x1p40f)));
        const int rare = odd[e] && !special[e];
        const float m = e ? main_r.y : main_r.x;
        ++g_n_atan2;
        g_rare += rare;
        g_special += special[e];
        if (special[e] != need_special || special_c[e] != need_special || (special[e] && !odd[e])) ++g_bad_flags;
        if (!odd[e] && !same(m, want)) ++g_bad_sound;
        if (!special[e] && (!same(e ? patched.y : patched.x, want) || !same(e ? composed.y : composed.x, want)))
            ++g_bad_composed;
        // the keyed table: same flags; same z wherever the quotient is below 2^25 (at or above, the result is the
        // patch's constant whichever row was read)
        if (oddk[e] != odd[e]) ++g_bad_keyed;
        if (!special[e] && fbits(e ? q.y : q.x) < 0x4c000000u && !same(e ? zk.y : zk.x, e ? z.y : z.x)) ++g_bad_keyed;
        if (rare) {
            const uint32_t ix = fbits(xa), iy = fbits(ya);
            const int k = ((int)iy - (int)ix) >> 23;
            int cls = -1;
            if (iy == 0) cls = kZeroY;
            else if (ix == 0) cls = kZeroX;
            else if (k > 26) cls = kGapBig;
            else if (k < -26 && (fbits(xe) >> 31)) cls = kGapNeg;
            else if (fbits(e ? q.y : q.x) >= 0x4c000000u) cls = kHuge;
            if (cls >= 0) {
                ++g_class_seen[cls];
                g_class_main_differs[cls] += !same(m, want);
            }
        }
    }
}

static void check_asin_pair(float x0, float x1) {
    const pbr_lv2 x = {x0, x1};
    int odd[2], special[2] = {0, 0}, special_c[2];
    const pbr_lv2 main_r = pbr_asinf_x2_main(x, odd);
    const pbr_lv2 patched = pbr_asinf_x2_patch(x, main_r, special);
    const pbr_lv2 composed = pbr_asinf_x2(x, special_c);
    for (int e = 0; e < 2; ++e) {
        const float xe = e ? x1 : x0;
        const float want = pbr_asinf(xe);
        const int need_special = fabsf(xe) > 1.0f || xe != xe;
        const int rare = odd[e] && !special[e];
        const float m = e ? main_r.y : main_r.x;
        ++g_n_asin;
        g_rare += rare;
        g_special += special[e];
        if (special[e] != need_special || special_c[e] != need_special || (special[e] && !odd[e])) ++g_bad_flags;
        if (rare != (fabsf(xe) == 1.0f)) ++g_bad_flags;
        if (!odd[e] && !same(m, want)) ++g_bad_sound;
        if (!special[e] && (!same(e ? patched.y : patched.x, want) || !same(e ? composed.y : composed.x, want)))
            ++g_bad_composed;
        if (rare) {
            ++g_class_seen[kAsinOne];
            g_class_main_differs[kAsinOne] += !same(m, want);
        }
    }
}

static const float kPartner = 0.4375f * 1.37f;  // an ordinary value to sit beside a directed one

static void atan2_directed(float y, float x) {
    check_atan2_pair(y, x, kPartner, 0.8f);   // first element
    check_atan2_pair(kPartner, -0.8f, y, x);  // second element
    check_atan2_pair(y, x, y, x);             // both
}
static void asin_directed(float x) {
    check_asin_pair(x, 0.3f);
    check_asin_pair(-0.7f, x);
    check_asin_pair(x, x);
}

static inline uint64_t mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// Random pair i: unit-box directions, some scaled towards 0 by up to 2^-63, exact zeros, and raw bit patterns.
static void random_pair(uint64_t i, float& y, float& x) {
    const uint64_t h = mix(0xa7a2 ^ (i * 0x100000001B3ull));
    const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
    const float a = (float)(lo >> 8) * 0x1p-23f - 1.0f, b = (float)(hi >> 8) * 0x1p-23f - 1.0f;
    const int sh = (int)((h >> 20) & 63);
    switch (i & 7) {
        case 0: y = bitsf(lo); x = bitsf(hi); break;
        case 1: y = (lo & 1) ? 0.0f : -0.0f; x = b; break;
        case 2: y = a; x = (hi & 1) ? 0.0f : -0.0f; break;
        case 3: y = ldexpf(a, -sh); x = b; break;
        case 4: y = a; x = ldexpf(b, -sh); break;
        default: y = a; x = b;
    }
}

int main(int argc, char** argv) {
    const uint64_t n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    const float zeros[2] = {0.0f, -0.0f};
    const float mags[] = {0.0f, 0x1p-40f, 0x1p-19f, 0.3f, 1.0f, 16.0f, 0x1p40f};
    // every combination of +-0 in either component, against zeros and ordinary magnitudes of both signs
    for (float zy : zeros)
        for (float m : mags)
            for (int s = 0; s < 2; ++s) {
                atan2_directed(zy, s ? -m : m);
                atan2_directed(s ? -m : m, zy);
            }
    // exponent gaps of exactly 26 and 27 (and their neighbours 25, 28), both orders, both x signs, with mantissas on
    // either side of the partner's (k = (iy - ix) >> 23 rounds down)
    for (int gap = 24; gap <= 28; ++gap)
        for (int s = 0; s < 2; ++s)
            for (float my : {1.0f, 1.25f, 1.9999999f})
                for (float mx : {1.0f, 1.5f}) {
                    const float sx = s ? -1.0f : 1.0f;
                    atan2_directed(ldexpf(my, gap - 10), sx * ldexpf(mx, -10));
                    atan2_directed(-ldexpf(my, -10), sx * ldexpf(mx, gap - 10));
                    atan2_directed(ldexpf(my, -10), sx * ldexpf(mx, gap - 10));
                }
    // atanf's five row thresholds with two neighbours on each side, and 2^25 +- 1 ulp, as quotients y / 1 and with
    // x = -1, +-2 (an exact quotient as well)
    for (uint32_t t : {0x3ee00000u, 0x3f300000u, 0x3f980000u, 0x401c0000u, 0x4c000000u})
        for (int d = -2; d <= 2; ++d)
            for (float x : {1.0f, -1.0f, 2.0f, -2.0f}) {
                atan2_directed(bitsf(t + (uint32_t)d) * fabsf(x), x);
                atan2_directed(-bitsf(t + (uint32_t)d) * fabsf(x), x);
            }
    // outside the window, infinities, NaN
    for (float v : {0x1p-41f, 0x1p41f, INFINITY, NAN, 0x1p-126f, 0x1p-149f})
        for (float o : {0.0f, 1.0f, -3.0f}) {
            atan2_directed(v, o);
            atan2_directed(o, v);
            atan2_directed(-v, o);
        }
    // asinf: |x| in {0.5, 0.975 (0x3f79999a), 1} with +-1 ulp, |x| > 1, NaN, zeros, the early-return range
    for (uint32_t t : {0x3f000000u, 0x3f79999au, 0x3f800000u})
        for (int d = -1; d <= 1; ++d) {
            asin_directed(bitsf(t + (uint32_t)d));
            asin_directed(-bitsf(t + (uint32_t)d));
        }
    for (float v : {1.5f, -2.0f, INFINITY, NAN, 0.0f, -0.0f, 0x1p-28f, -0x1p-30f, 0x1p-126f})
        asin_directed(v);
    const uint64_t n_directed = g_n_atan2 + g_n_asin;
    // the seeded random sample
    for (uint64_t i = 0; i < n_random; i += 2) {
        float y0, x0, y1, x1;
        random_pair(i, y0, x0);
        random_pair(i + 1, y1, x1);
        check_atan2_pair(y0, x0, y1, x1);
        if ((i & 6) == 0) check_asin_pair(y0 < -1.0f || y0 > 1.0f ? x1 : y0, x1);
    }
    printf("directed_elements %llu\n", (unsigned long long)n_directed);
    printf("atan2_elements %llu\nasin_elements %llu\n", (unsigned long long)g_n_atan2, (unsigned long long)g_n_asin);
    printf("rare_elements %llu\nspecial_elements %llu\n", (unsigned long long)g_rare, (unsigned long long)g_special);
    for (int c = 0; c < kClasses; ++c)
        printf("class_%s %llu main_differs %llu\n", kClassName[c], (unsigned long long)g_class_seen[c],
               (unsigned long long)g_class_main_differs[c]);
    printf("bad_soundness %llu\nbad_flags %llu\nbad_composed %llu\nbad_keyed %llu\n", (unsigned long long)g_bad_sound,
           (unsigned long long)g_bad_flags, (unsigned long long)g_bad_composed, (unsigned long long)g_bad_keyed);
    return (g_bad_sound | g_bad_flags | g_bad_composed | g_bad_keyed) != 0;
}
