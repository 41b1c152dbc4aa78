"""pbr_blend_layer (csrc/blend_layer.h; the transparent PSO's output merger, PBRApp.cpp:831-842) restated in numpy
float32, one numpy operation per specified operation. A helper, not a test.

    blend(src (H, W, 4) float32, alpha (H, W) float32, coverage (H, W) uint8, dst) -> the blended copy of dst

``dst`` (H, W, 4) float32 is RGBA32F, uint8 is RGBA8_UNORM."""
import numpy as np

F = np.float32


def saturate_input(v):
    """The fixed-point render-target rule for a blend input: NaN -> 0, clamp to [0, 1]."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        c = np.where(v > F(1), F(1), v)
        c = np.where(c < F(0), F(0), c)
    return np.where(np.isnan(v), F(0), c).astype(F)


def unorm8(c):
    """The library's FLOAT -> UNORM rule (pbr_output_format): NaN -> 0, clamp to [0, 1], c * 255 + 0.5, truncate."""
    c = saturate_input(c)
    return ((c * F(255.0)).astype(F) + F(0.5)).astype(F).astype(np.uint8)


def blend(src, alpha, coverage, dst):
    src, a = np.asarray(src, F), np.asarray(alpha, F)
    out = dst.copy()
    on = np.asarray(coverage) != 0
    with np.errstate(all="ignore"):
        if dst.dtype == np.uint8:
            a = saturate_input(a)
            for c in range(3):
                d = (dst[..., c].astype(F) / F(255.0)).astype(F)
                s = saturate_input(src[..., c])
                out[..., c][on] = unorm8(((s * a).astype(F) + (d * (F(1.0) - a).astype(F)).astype(F)).astype(F))[on]
            out[..., 3][on] = unorm8(a)[on]
        else:
            for c in range(3):
                d = dst[..., c]
                out[..., c][on] = ((src[..., c] * a).astype(F) + (d * (F(1.0) - a).astype(F)).astype(F)).astype(F)[on]
            out[..., 3][on] = a[on]
    return out
