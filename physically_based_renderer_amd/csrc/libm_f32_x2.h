/* libm_f32_x2.h -- WorldToSkyUV's atan2f and asinf (libm_f32.h: glibc 2.35's flt-32 e_atan2f.c + s_atanf.c and
 * e_asinf.c) for a PAIR of arguments at once, without branches, bit for bit the same as the scalar restatement.
 *
 * Why: the scalar functions branch on the argument's range (atanf: five reduction intervals, each with its own
 * IEEE division; asinf: two regimes and a sub-case). With the uncorrelated normals of a G-buffer every branch
 * runs in every wave, one pixel at a time: the diffuse-IBL block was 1,054 VALU instructions per wave of the
 * headline kernel (14% of all; tools/variant_pmc.sh). Here every interval's operands are selected
 * per element first and ONE chain of operations runs for both pixels in packed fp32 (v_pk_mul/add/fma_f32): the
 * same IEEE operations in the same order as the branch the element would have taken, so the same bits:
 *   atanf reduction x' = RN(RN(A x) - C) / RN(RN(C x) + A), rounded as the branch rounds it (table rows below):
 *     |x| < 7/16: A = 1, C = 0 -> x / 1 = x;  < 11/16: (2x - 1) / (x + 2);  < 19/16: (x - 1) / (x + 1);
 *     < 39/16: (x - 1.5) / (1.5x + 1);  else: (0x - 1) / (x + 0) = -1 / x   (RN(A x) is exact or the branch's own
 *     product, and adding 0 or multiplying by 1 changes nothing);
 *   result hi - ((x' S - lo) - x'), which for the first interval (hi = lo = 0) is RN(x' - RN(x' S)), the branch's
 *   x - x S, by the symmetry of round-to-nearest.
 *
 * Main path and patch. Each function is split in two. The MAIN part assumes the ordinary argument --
 * atan2f: both components nonzero and inside the window, the quotient's magnitude in (2^-26, 2^25); asinf:
 * |x| < 1 -- and carries no select for anything else; it reports per element whether the argument was `odd` (not
 * ordinary). The PATCH part holds the selects of the remaining cases (a zero component, the exponent-gap shortcuts
 * |k| > 26, a quotient at or above 2^25, |x| == 1). The caller runs the patch inside one wave-uniform branch, only
 * when some element is odd; an odd element is then either `rare` (the patch gives glibc's bits) or `special` (NaN or
 * infinite components, nonzero magnitudes outside [2^-40, 2^40] for atan2f, |x| > 1 for asinf: the caller takes the
 * scalar functions for those). On an odd element the main part computes with harmless values (a division by zero,
 * the square root of zero: a NaN or an infinity at worst, which the patch replaces). pbr_atan2f_x2 / pbr_asinf_x2
 * compose main and patch per pair; tests/hip/libm_probe.hip and tools/libm_x2_check.cpp compare them with glibc.
 *
 * Divisions and the square root: on the device the exact fast sequences (Markstein division on a v_rcp + Newton
 * reciprocal, rsq + Newton sqrt), whose operands stay inside their proven windows on ordinary elements (comments
 * below); the host build (LIBM_F32_HOST, the CPU check) uses IEEE / and sqrtf, which those sequences equal in the
 * window.
 */
#ifndef PBR_LIBM_F32_X2_H
#define PBR_LIBM_F32_X2_H

#include "libm_f32.h"

typedef float pbr_lv2 __attribute__((ext_vector_type(2)));

#ifdef LIBM_F32_HOST
#define PBR_LX2_FN static inline
PBR_LX2_FN pbr_lv2 pbr_lx2_div(pbr_lv2 a, pbr_lv2 b) { return a / b; }
PBR_LX2_FN pbr_lv2 pbr_lx2_sqrt(pbr_lv2 a) { return (pbr_lv2){sqrtf(a.x), sqrtf(a.y)}; }
#else
#define PBR_LX2_FN __device__ __forceinline__
/* a / b, correctly rounded, for b in [2^-60, 2^60], a == 0 or |a| in [2^-96, 2^60], |a / b| in [2^-120, 2^120]
 * (pbr_device_math.h: recip_nr is RN(1/b) there, and the Markstein step gives RN(a/b)). */
PBR_LX2_FN pbr_lv2 pbr_lx2_div(pbr_lv2 a, pbr_lv2 b) {
    const pbr_lv2 r0 = (pbr_lv2){__builtin_amdgcn_rcpf(b.x), __builtin_amdgcn_rcpf(b.y)};
    const pbr_lv2 e = __builtin_elementwise_fma(-b, r0, (pbr_lv2)(1.0f));
    const pbr_lv2 r = __builtin_elementwise_fma(e, r0, r0);
    const pbr_lv2 q = a * r;
    const pbr_lv2 t = __builtin_elementwise_fma(b, q, -a);
    return __builtin_elementwise_fma(-t, r, q);
}
/* sqrtf for exponents in [-64, 64] (pbr_device_math.h sqrt_nr, probed on gfx950). */
PBR_LX2_FN pbr_lv2 pbr_lx2_sqrt(pbr_lv2 x) {
    const pbr_lv2 y = (pbr_lv2){__builtin_amdgcn_rsqf(x.x), __builtin_amdgcn_rsqf(x.y)};
    const pbr_lv2 s0 = x * y;
    const pbr_lv2 r = __builtin_elementwise_fma(-s0, s0, x);
    return __builtin_elementwise_fma(r, 0.5f * y, s0);
}
#endif

PBR_LX2_FN pbr_lv2 pbr_lx2_sel(int c0, int c1, pbr_lv2 a, pbr_lv2 b) {
    return (pbr_lv2){c0 ? a.x : b.x, c1 ? a.y : b.y};
}
PBR_LX2_FN pbr_lv2 pbr_lx2_abs(pbr_lv2 a) { return (pbr_lv2){PBR_LM_FABSF(a.x), PBR_LM_FABSF(a.y)}; }

/* s_atanf.c's reduction intervals as table rows {A, C, hi, lo}: the branch for |x| in [7/16, 11/16) computes
 * (2x - 1) / (x + 2), [11/16, 19/16) (x - 1) / (x + 1), [19/16, 39/16) (x - 1.5) / (1.5x + 1), [39/16, 2^25)
 * -1 / x, i.e. RN(RN(A x) - C) / RN(RN(C x) + A) with the row's A, C; row 4 (A = 1, C = 0: x / 1 = x, hi = lo = 0)
 * stands for |x| < 7/16 and, with its result replaced by the constant, for |x| >= 2^25. */
typedef struct __attribute__((aligned(16))) {
    float a, c, hi, lo;
} pbr_atan_seg;
#define PBR_ATAN_SEG_ROW0 {2.0f, 1.0f, 4.6364760399e-01f, 5.0121582440e-09f}
#define PBR_ATAN_SEG_ROW1 {1.0f, 1.0f, 7.8539812565e-01f, 3.7748947079e-08f}
#define PBR_ATAN_SEG_ROW2 {1.0f, 1.5f, 9.8279368877e-01f, 3.4473217170e-08f}
#define PBR_ATAN_SEG_ROW3 {0.0f, 1.0f, 1.5707962513e+00f, 7.5497894159e-08f}
#define PBR_ATAN_SEG_ROW4 {1.0f, 0.0f, 0.0f, 0.0f}
#define PBR_ATAN_SEG_TABLE_INIT \
    {PBR_ATAN_SEG_ROW0, PBR_ATAN_SEG_ROW1, PBR_ATAN_SEG_ROW2, PBR_ATAN_SEG_ROW3, PBR_ATAN_SEG_ROW4}

/* The row without a compare chain. The four interval thresholds 0x3ee00000 (7/16), 0x3f300000 (11/16), 0x3f980000
 * (19/16) and 0x401c0000 (39/16) are multiples of 2^18 (the last one of no higher power), so the row is a function
 * of the key
 *   key(ia) = min(max((ia >> 18) - 0xfb7, 0), 80):   0: below 7/16 (row 4)   1..20: row 0   21..46: row 1
 *                                                     47..79: row 2           80: at or above 39/16 (row 3)
 * The device keeps the 16-byte rows laid out BY KEY in LDS (PBR_ATAN_SEG_KEYED_INIT: 81 rows; pbr_device_math.h
 * load_libm_tables) and reads row `key` directly: a shift, a saturating subtract and a minimum per element instead
 * of five compares and their sums. Callers with the five-row table (the probes and the host check) get the row
 * index from the key by counting the interval starts at or below it (popcounts under constant masks). |x| >= 2^25
 * is the separate case: its result is the constant, whichever row was read (the keyed table reads row 3 there, the
 * five-row index says 4 as it always did). */
#define PBR_ATAN_KEYS 81
#define PBR_LX2_REP2(...) __VA_ARGS__, __VA_ARGS__ /* variadic: a row's braces hold commas */
#define PBR_LX2_REP4(...) PBR_LX2_REP2(__VA_ARGS__), PBR_LX2_REP2(__VA_ARGS__)
#define PBR_LX2_REP8(...) PBR_LX2_REP4(__VA_ARGS__), PBR_LX2_REP4(__VA_ARGS__)
#define PBR_LX2_REP16(...) PBR_LX2_REP8(__VA_ARGS__), PBR_LX2_REP8(__VA_ARGS__)
#define PBR_ATAN_SEG_KEYED_INIT                                                                                     \
    {PBR_ATAN_SEG_ROW4,                                                                      /* key 0 */            \
     PBR_LX2_REP16(PBR_ATAN_SEG_ROW0), PBR_LX2_REP4(PBR_ATAN_SEG_ROW0),                     /* keys 1..20 */       \
     PBR_LX2_REP16(PBR_ATAN_SEG_ROW1), PBR_LX2_REP8(PBR_ATAN_SEG_ROW1), PBR_LX2_REP2(PBR_ATAN_SEG_ROW1), /* 21..46 */ \
     PBR_LX2_REP16(PBR_ATAN_SEG_ROW2), PBR_LX2_REP16(PBR_ATAN_SEG_ROW2), PBR_ATAN_SEG_ROW2, /* keys 47..79 */      \
     PBR_ATAN_SEG_ROW3}                                                                      /* key 80 */

PBR_LX2_FN uint32_t pbr_lx2_atan_key(uint32_t ia) {
    const uint32_t d = __builtin_elementwise_sub_sat(ia >> 18, 0xfb7u); /* saturating: v_sub_u32 ... clamp */
    return d < (uint32_t)(PBR_ATAN_KEYS - 1) ? d : (uint32_t)(PBR_ATAN_KEYS - 1);
}
/* The five-row table's row for |x| (bit pattern ia, finite): 0..3 as above, 4 below 7/16 or at/above 2^25. */
PBR_LX2_FN int pbr_lx2_atan_row(uint32_t ia) {
    const uint32_t key = pbr_lx2_atan_key(ia);
    /* the keys where a row begins (1, 21, 47 | 80), and the keys at or below `key`, as two 64-bit words */
    const uint64_t starts_lo = (1ull << 1) | (1ull << 21) | (1ull << 47), starts_hi = 1ull << (80 - 64);
    const uint64_t below_lo = (2ull << (key < 63u ? key : 63u)) - 1ull;
    const uint64_t below_hi = key < 64u ? 0ull : (2ull << (key - 64u)) - 1ull;
    const int c = __builtin_popcountll(starts_lo & below_lo) + __builtin_popcountll(starts_hi & below_hi); /* 0..4 */
    const int row = (int)((0x32104u >> (4 * c)) & 7u); /* c == 0 -> 4, else c - 1 */
    return ia >= 0x4c000000u ? 4 : row;
}
/* The row for |x|: `keyed` (a compile-time constant at every call) says which layout `tab` has. */
PBR_LX2_FN pbr_atan_seg pbr_lx2_atan_seg_of(uint32_t ia, const pbr_atan_seg* tab, int keyed) {
    return keyed ? tab[pbr_lx2_atan_key(ia)] : tab[pbr_lx2_atan_row(ia)];
}

/* atanf(a) of s_atanf.c for a pair of finite a in [0, 2^25), branch-free (main part: a >= 2^25 is the patch's).
 * Division window: the denominators are 1, x + 2, x + 1, 1.5x + 1 or x in [2.4375, 2^25) -- inside [1, 2^25]; the
 * numerators 0, -1, multiples of 2^-24 of magnitude <= 1, or x itself on row 4 (the caller keeps x == 0 or
 * >= 2^-81). */
PBR_LX2_FN pbr_lv2 pbr_atanf_pos_x2_main(pbr_lv2 a, const pbr_atan_seg* tab, int keyed) {
    PBR_LM_NO_CONTRACT
    const float a0 = 3.3333334327e-01f, a1 = -2.0000000298e-01f, a2 = 1.4285714924e-01f, a3 = -1.1111110449e-01f,
                a4 = 9.0908870101e-02f, a5 = -7.6918758452e-02f, a6 = 6.6610731184e-02f, a7 = -5.8335702866e-02f,
                a8 = 4.9768779427e-02f, a9 = -3.6531571299e-02f, a10 = 1.6285819933e-02f;
    const pbr_atan_seg g0 = pbr_lx2_atan_seg_of(pbr_lm_bits(a.x), tab, keyed),
                       g1 = pbr_lx2_atan_seg_of(pbr_lm_bits(a.y), tab, keyed);
    const pbr_lv2 A = {g0.a, g1.a}, C = {g0.c, g1.c};
    const pbr_lv2 x = pbr_lx2_div(A * a - C, C * a + A);
    const pbr_lv2 z = x * x;
    const pbr_lv2 w = z * z;
    const pbr_lv2 s1 = z * (a0 + w * (a2 + w * (a4 + w * (a6 + w * (a8 + w * a10)))));
    const pbr_lv2 s2 = w * (a1 + w * (a3 + w * (a5 + w * (a7 + w * a9))));
    const pbr_lv2 H = {g0.hi, g1.hi}, L = {g0.lo, g1.lo};
    return H - ((x * (s1 + s2) - L) - x);
}
/* The patch for a >= 2^25: atanhi[3] + atanlo[3], rounded once. */
PBR_LX2_FN pbr_lv2 pbr_atanf_pos_x2_patch(pbr_lv2 a, pbr_lv2 r) {
    const float huge = 1.5707962513e+00f + 7.5497894159e-08f;
    return pbr_lx2_sel(pbr_lm_bits(a.x) >= 0x4c000000u, pbr_lm_bits(a.y) >= 0x4c000000u, (pbr_lv2)(huge), r);
}
/* Main and patch composed (the five-row table): atanf for every finite a >= 0. */
PBR_LX2_FN pbr_lv2 pbr_atanf_pos_x2(pbr_lv2 a, const pbr_atan_seg* tab) {
    return pbr_atanf_pos_x2_patch(a, pbr_atanf_pos_x2_main(a, tab, 0));
}

/* ---- atan2f(y, x) of e_atan2f.c for a pair ------------------------------------------------------------------------
 * Head (main): q = |y / x| and z = atanf(q) for the ordinary element, and odd[e] = 1 unless both components are
 * nonzero with magnitudes in [2^-40, 2^40] and q is in (2^-26, 2^25). The quotient test covers the exponent-gap
 * shortcuts: with k = (iy - ix) >> 23 on the bit patterns, k > 26 means |y / x| >= 2^26 and k < -26 means
 * |y / x| < 2^-26, whose rounded quotient is at most 2^-26 (so `odd` is set on every |k| > 26 element, and on a few
 * neighbours with k == -26 or x > 0 that the patch leaves as they are). A zero x makes the device's quotient a NaN
 * and the host's an infinity or a NaN: both fail the test; a zero component fails the window test as well. */
PBR_LX2_FN pbr_lv2 pbr_atan2f_x2_head(pbr_lv2 y, pbr_lv2 x, int odd[2], pbr_lv2* q_abs, const pbr_atan_seg* tab,
                                      int keyed) {
    const pbr_lv2 q = pbr_lx2_abs(pbr_lx2_div(y, x)); /* in [2^-80, 2^80] when both are in [2^-40, 2^40] */
    const uint32_t iq[2] = {pbr_lm_bits(q.x), pbr_lm_bits(q.y)};
    const uint32_t ix[2] = {pbr_lm_bits(x.x) & 0x7fffffffu, pbr_lm_bits(x.y) & 0x7fffffffu};
    const uint32_t iy[2] = {pbr_lm_bits(y.x) & 0x7fffffffu, pbr_lm_bits(y.y) & 0x7fffffffu};
    for (int e = 0; e < 2; ++e) {
        /* unsigned wrap: one compare per window; 0x2b800000 = 2^-40, 0x53800000 = 2^40, 0x32800000 = 2^-26 */
        const int in_x = ix[e] - 0x2b800000u <= 0x53800000u - 0x2b800000u;
        const int in_y = iy[e] - 0x2b800000u <= 0x53800000u - 0x2b800000u;
        const int in_q = iq[e] - 0x32800001u < 0x4c000000u - 0x32800001u;
        odd[e] = !(in_x & in_y & in_q);
    }
    *q_abs = q;
    return pbr_atanf_pos_x2_main(q, tab, keyed);
}
/* Tail (main): the quadrant of e_atan2f.c's switch on m = sign(y) + 2 sign(x). z >= +0 here, so
 *   m = 0: z   m = 1: -z   m = 2: pi - (z - pi_lo)   m = 3: (z - pi_lo) - pi = -(pi - (z - pi_lo))
 * (round-to-nearest is symmetric and pi - (z - pi_lo) >= pi/2 is never zero): the magnitude is chosen by x's sign
 * and y's sign bit is put on it. */
PBR_LX2_FN pbr_lv2 pbr_atan2f_x2_tail(pbr_lv2 y, pbr_lv2 x, pbr_lv2 z) {
    PBR_LM_NO_CONTRACT
    const float pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const pbr_lv2 q2 = pi - (z - pi_lo);
    const pbr_lv2 mag = pbr_lx2_sel(pbr_lm_bits(x.x) >> 31, pbr_lm_bits(x.y) >> 31, q2, z);
    return (pbr_lv2){pbr_lm_float(pbr_lm_bits(mag.x) ^ (pbr_lm_bits(y.x) & 0x80000000u)),
                     pbr_lm_float(pbr_lm_bits(mag.y) ^ (pbr_lm_bits(y.y) & 0x80000000u))};
}
/* Tail with the patch, in place of pbr_atan2f_x2_tail when an element of the wave is odd: e_atan2f.c's remaining
 * cases as selects, in its order. q >= 2^25: atanf's constant; k > 26: pi/2 + pi_lo/2; x < 0 and k < -26: 0; then
 * the quadrant; then x == +-0: +-pi/2 by y's sign; y == +-0: y itself, or +-pi by x's sign. Ordinary elements pass
 * through every select unchanged. */
PBR_LX2_FN pbr_lv2 pbr_atan2f_x2_tail_patch(pbr_lv2 y, pbr_lv2 x, pbr_lv2 q_abs, pbr_lv2 z) {
    PBR_LM_NO_CONTRACT
    const float pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f, tiny = 1.0e-30f;
    const float big_z = pi_o_2 + 0.5f * pi_lo; /* k > 26 */
    const float c_pi = pi + tiny, c_npi = -pi - tiny, c_pio2 = pi_o_2 + tiny, c_npio2 = -pi_o_2 - tiny;
    const uint32_t hx[2] = {pbr_lm_bits(x.x), pbr_lm_bits(x.y)}, hy[2] = {pbr_lm_bits(y.x), pbr_lm_bits(y.y)};
    int xneg[2], kbig[2], kneg[2], yz[2], xz[2];
    for (int e = 0; e < 2; ++e) {
        const uint32_t ix = hx[e] & 0x7fffffffu, iy = hy[e] & 0x7fffffffu;
        const int k = ((int)iy - (int)ix) >> 23;
        xneg[e] = (int)(hx[e] >> 31);
        kbig[e] = k > PBR_ATAN2F_KMAX;
        kneg[e] = xneg[e] && k < -PBR_ATAN2F_KMAX;
        yz[e] = iy == 0;
        xz[e] = ix == 0;
    }
    z = pbr_atanf_pos_x2_patch(q_abs, z);
    z = pbr_lx2_sel(kbig[0], kbig[1], (pbr_lv2)(big_z), z);
    z = pbr_lx2_sel(kneg[0], kneg[1], (pbr_lv2)(0.0f), z);
    pbr_lv2 r = pbr_atan2f_x2_tail(y, x, z);
    const pbr_lv2 r_xz = pbr_lx2_sel(hy[0] >> 31, hy[1] >> 31, (pbr_lv2)(c_npio2), (pbr_lv2)(c_pio2));
    const pbr_lv2 r_yz = pbr_lx2_sel(!xneg[0], !xneg[1], y, pbr_lx2_sel(hy[0] >> 31, hy[1] >> 31, (pbr_lv2)(c_npi),
                                                                        (pbr_lv2)(c_pi)));
    r = pbr_lx2_sel(xz[0], xz[1], r_xz, r);
    return pbr_lx2_sel(yz[0], yz[1], r_yz, r);
}
/* special[e] = 1 where element e needs the scalar function: a NaN or infinite component, or a nonzero magnitude
 * outside [2^-40, 2^40]. (An odd element that is not special is `rare`: the patch covers it.) */
PBR_LX2_FN void pbr_atan2f_x2_special(pbr_lv2 y, pbr_lv2 x, int special[2]) {
    const uint32_t ix[2] = {pbr_lm_bits(x.x) & 0x7fffffffu, pbr_lm_bits(x.y) & 0x7fffffffu};
    const uint32_t iy[2] = {pbr_lm_bits(y.x) & 0x7fffffffu, pbr_lm_bits(y.y) & 0x7fffffffu};
    for (int e = 0; e < 2; ++e) {
        const int in_x = ix[e] == 0 || (ix[e] >= 0x2b800000u && ix[e] <= 0x53800000u); /* 0 or [2^-40, 2^40] */
        const int in_y = iy[e] == 0 || (iy[e] >= 0x2b800000u && iy[e] <= 0x53800000u);
        special[e] = !(in_x && in_y);
    }
}
/* Main and patch composed: atan2f(y, x) for a pair, the patch when either element is odd (as the kernel runs it
 * when any element of the wave is). Covered: y == +-0, x == +-0, x == 1 (atanf(y) there: the same value through
 * this path), |k| > 26 (the exponent-gap shortcuts), the quadrants. `tab` is the five-row table. */
PBR_LX2_FN pbr_lv2 pbr_atan2f_x2(pbr_lv2 y, pbr_lv2 x, int special[2], const pbr_atan_seg* tab) {
    int odd[2];
    pbr_lv2 q;
    const pbr_lv2 z = pbr_atan2f_x2_head(y, x, odd, &q, tab, 0);
    pbr_atan2f_x2_special(y, x, special);
    return (odd[0] | odd[1]) ? pbr_atan2f_x2_tail_patch(y, x, q, z) : pbr_atan2f_x2_tail(y, x, z);
}

/* ---- asinf(x) of e_asinf.c for a pair -----------------------------------------------------------------------------
 * Main: both regimes of |x| < 1 evaluated and selected; odd[e] = 1 for |x| >= 1 or NaN. Windows: below 0.5, no
 * division; above, t = (1 - |x|) / 2 in [2^-25, 0.25] (sqrt exponent >= -25), s + w in [2^-13, 1], t - w^2
 * exact-ish and >= 0 (0 or >= 2^-50). Lanes of the other regime compute with harmless values (t in (0.25, 0.5]
 * below 0.5; t == 0 at |x| == 1, whose result the patch replaces). */
PBR_LX2_FN pbr_lv2 pbr_asinf_x2_main(pbr_lv2 x, int odd[2]) {
    PBR_LM_NO_CONTRACT
    const float pio2_hi = 1.57079637050628662109375f, pio2_lo = -4.37113900018624283e-8f,
                pio4_hi = 0.785398185253143310546875f;
    const float p0 = 1.666675248e-1f, p1 = 7.495297643e-2f, p2 = 4.547037598e-2f, p3 = 2.417951451e-2f,
                p4 = 4.216630880e-2f;
    const uint32_t hx[2] = {pbr_lm_bits(x.x), pbr_lm_bits(x.y)};
    const uint32_t ix[2] = {hx[0] & 0x7fffffffu, hx[1] & 0x7fffffffu};
    odd[0] = ix[0] >= 0x3f800000u;
    odd[1] = ix[1] >= 0x3f800000u;
    /* |x| < 0.5 (below 2^-27 this is x itself, as the scalar function's early return) */
    const pbr_lv2 ts = x * x;
    const pbr_lv2 ws = ts * (p0 + ts * (p1 + ts * (p2 + ts * (p3 + ts * p4))));
    const pbr_lv2 r_small = x + x * ws;
    /* 0.5 <= |x| < 1 */
    const pbr_lv2 wl = 1.0f - pbr_lx2_abs(x);
    const pbr_lv2 t = wl * 0.5f;
    const pbr_lv2 p = t * (p0 + t * (p1 + t * (p2 + t * (p3 + t * p4))));
    const pbr_lv2 s = pbr_lx2_sqrt(t);
    const pbr_lv2 r_far = pio2_hi - (2.0f * (s + s * p) - pio2_lo); /* |x| >= 0.975 */
    const pbr_lv2 w = (pbr_lv2){pbr_lm_float(pbr_lm_bits(s.x) & 0xfffff000u), pbr_lm_float(pbr_lm_bits(s.y) & 0xfffff000u)};
    const pbr_lv2 c = pbr_lx2_div(t - w * w, s + w);
    const pbr_lv2 pp = 2.0f * s * p - (pio2_lo - 2.0f * c);
    const pbr_lv2 q = pio4_hi - 2.0f * w;
    const pbr_lv2 r_mid = pio4_hi - (pp - q);
    pbr_lv2 r = pbr_lx2_sel(ix[0] >= 0x3f79999au, ix[1] >= 0x3f79999au, r_far, r_mid);
    /* x's sign on the (non-negative or NaN) result: the scalar function's -r, as a bit operation */
    r = (pbr_lv2){pbr_lm_float(pbr_lm_bits(r.x) ^ (hx[0] & 0x80000000u)), pbr_lm_float(pbr_lm_bits(r.y) ^ (hx[1] & 0x80000000u))};
    return pbr_lx2_sel(ix[0] < 0x3f000000u, ix[1] < 0x3f000000u, r_small, r);
}
/* Patch: |x| == 1 takes its own formula x pio2_hi + x pio2_lo. special[e] = 1 for |x| > 1 or NaN (the scalar
 * function's (x - x) / (x - x)). */
PBR_LX2_FN pbr_lv2 pbr_asinf_x2_patch(pbr_lv2 x, pbr_lv2 r, int special[2]) {
    PBR_LM_NO_CONTRACT
    const float pio2_hi = 1.57079637050628662109375f, pio2_lo = -4.37113900018624283e-8f;
    const uint32_t ix[2] = {pbr_lm_bits(x.x) & 0x7fffffffu, pbr_lm_bits(x.y) & 0x7fffffffu};
    special[0] = ix[0] > 0x3f800000u;
    special[1] = ix[1] > 0x3f800000u;
    const pbr_lv2 r_one = x * pio2_hi + x * pio2_lo;
    return pbr_lx2_sel(ix[0] == 0x3f800000u, ix[1] == 0x3f800000u, r_one, r);
}
/* Main and patch composed: asinf for a pair, special[e] = 1 for |x| > 1 or NaN. */
PBR_LX2_FN pbr_lv2 pbr_asinf_x2(pbr_lv2 x, int special[2]) {
    int odd[2];
    const pbr_lv2 r = pbr_asinf_x2_main(x, odd);
    if (odd[0] | odd[1]) return pbr_asinf_x2_patch(x, r, special);
    special[0] = special[1] = 0;
    return r;
}

#endif /* PBR_LIBM_F32_X2_H */
