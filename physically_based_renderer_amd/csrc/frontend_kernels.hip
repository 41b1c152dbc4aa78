// frontend_kernels.hip -- gfx950 kernels of the front end, which turns meshes and materials into the G-buffer the
// shading kernels read: the rasteriser (raster.h; pbr_rasterize) and the material resolve (material_resolve.h;
// pbr_resolve_materials); and the blend of a shaded transparent layer over the frame (blend_layer.h; pbr_blend_layer).
// raster.h states each rule of DESIGN.md §12 once where that leaves every kernel of this unit as it was (its header
// lists what stays apart and the comparison that decided it). A unit of its own, so a front-end change never
// recompiles the shading kernels. The Makefile gives it the flags these kernels were first built and measured
// under: the canonical fp32 flags and the max-ILP machine scheduler.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pbr_device_math.h"
#include "frontend_kernels.h"
#include "material_resolve.h"
#include "raster.h"
#include "blend_layer.h"
#include "msaa_resolve.h"

namespace pbr {

// This unit's copy of g_bounds_flags (pbr_debug_bounds.h); arm_bounds publishes the device's buffer to every unit.
hipError_t debug_bounds_publish_frontend(uint32_t* buf) {
#if PBR_DEBUG_BOUNDS
    return hipMemcpyToSymbol(HIP_SYMBOL(g_bounds_flags), &buf, sizeof(buf));
#else
    (void)buf;
    return hipErrorNotSupported;
#endif
}

}  // namespace pbr

// This unit's build record (pbr_build_info.h, pbr_build_info).
#include "pbr_build_info.h"
extern "C" __attribute__((used, visibility("default"))) const char pbr_unit_info_frontend_kernels[] =
    PBR_UNIT_INFO("frontend_kernels", PBR_BI_SWITCH(PBR_DEBUG_BOUNDS));
