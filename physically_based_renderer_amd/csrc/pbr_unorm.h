// pbr_unorm.h -- the library's FLOAT -> UNORM8 rule, one definition for every kernel that writes an R8G8B8A8_UNORM
// target: the shading kernels' stores (shade_pixel.h) and the layer blend (blend_layer.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pbr {

// D3D FLOAT -> UNORM8 (the R8G8B8A8_UNORM back buffer, d3dApp.h:124): NaN -> 0, clamp to [0, 1],
// c * 255 + 0.5 in fp32 (no contraction), truncate.
__device__ __forceinline__ uint32_t unorm8(float c) {
    if (!(c == c)) return 0u;
    c = c > 1.0f ? 1.0f : c;
    c = c < 0.0f ? 0.0f : c;
    return (uint32_t)(c * 255.0f + 0.5f);
}

}  // namespace pbr
