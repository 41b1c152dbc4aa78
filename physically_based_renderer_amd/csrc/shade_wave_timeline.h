// shade_wave_timeline.h -- development instrumentation of the pair kernels: per-wave clock stamps (PBR_WAVE_TIMELINE,
// tools/wave_timeline.py). The TL_* macros expand to nothing in every other build. g_wave_tl is one copy per
// translation unit: debug_wave_timeline (shade_kernels.hip) points every unit's copy at the same device buffer.
#pragma once
#include <hip/hip_runtime.h>

namespace pbr {

#ifndef PBR_WAVE_TIMELINE
#define PBR_WAVE_TIMELINE 0  // development build: per-wave clock stamps of the pair kernels (pbr_debug_wave_timeline)
#endif
#if PBR_WAVE_TIMELINE
// kTlWords per wave (wave = block * 4 + wave in block): [0] HW_ID | XCC_ID << 32, [1] entry, [2] G-buffer pair
// arrived, [3] light loops start, [4] light loops end, [5] stores issued (s_memrealtime, 100 MHz, one clock for
// the whole chip), [6] / [7] s_memtime (shader clock) at entry / at the end. Lane 0 stores them (vector stores).
constexpr int kTlWords = 8;
static __device__ unsigned long long* g_wave_tl;
static __device__ long long g_wave_tl_cap;
#define TL_RT(i_) (tl[i_] = (unsigned long long)__builtin_amdgcn_s_memrealtime())
#define TL_BEGIN()                                                                                           \
    unsigned long long tl[kTlWords];                                                                         \
    TL_RT(1);                                                                                                \
    tl[6] = (unsigned long long)__builtin_amdgcn_s_memtime();                                                \
    tl[0] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) |                                            \
            ((unsigned long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32)
#define TL_LOADED()                                      \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    TL_RT(2)
#define TL_FLAGS(f_) (tl[0] |= (unsigned long long)(f_) << 48)  // bits 48+: kernel-specific wave flags
#define TL_END(wv_)                                                                     \
    do {                                                                                \
        TL_RT(5);                                                                       \
        tl[7] = (unsigned long long)__builtin_amdgcn_s_memtime();                       \
        const long long w_ = (wv_);                                                     \
        if ((threadIdx.x & 63) == 0 && g_wave_tl != nullptr && w_ < g_wave_tl_cap) {    \
            for (int i_ = 0; i_ < kTlWords; ++i_) g_wave_tl[w_ * kTlWords + i_] = tl[i_]; \
        }                                                                               \
    } while (0)
#else
#define TL_BEGIN()
#define TL_FLAGS(f_)
#define TL_LOADED()
#define TL_RT(i_)
#define TL_END(wv_)
#endif

}  // namespace pbr
