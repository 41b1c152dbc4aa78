"""The front end's negative control for tests/test_gpu_debug_bounds.py. A helper, not a test: run as a script in a
child process (`python tests/frontend_skew_cases.py OUT.npz`) under the bounds-checked build (PBR_LIB_PATH) with
PBR_DEBUG_BOUNDS_SKEW=1, it rasterises one raster_cases case at 70x37 and resolves the smallest textured resolve_cases
case (70x3), and stores the pbr_debug_bounds report after each: int64 per class of CLASSES, the last offending index,
-1 where the class was clean. Under the skew the host hands the checks an index count and a texel count of 0, so the
front end's kernel unit must flag "mesh" and "texel" -- if its flag pointer was published (pbr_context.hip, arm_bounds).
The pixel values under the skew are not looked at (a flagged index reads element 0)."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLASSES = ("gbuffer", "output", "coverage", "texel", "light", "lds", "raster", "mesh")
RASTER_CASE, RASTER_FRAME = "one_triangle", "70x37"
RESOLVE_SHAPE = (3, 70)


def main(out_path):
    import raster_cases
    import resolve_cases
    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd.renderer import ShadingContext

    report = lambda flagged: np.array([flagged.get(k, -1) for k in CLASSES], np.int64)
    result = {}
    with ShadingContext(0) as ctx:
        ctx.debug_bounds(reset=True)
        W, H = raster_cases.FRAMES[RASTER_FRAME]
        raster_cases.device_rasterize(ctx, *raster_cases.case(RASTER_CASE, W, H))
        result["rasterize"] = report(ctx.debug_bounds(reset=True))
        mats, texs = resolve_cases.table()
        attrs, ids = resolve_cases.attributes(*RESOLVE_SHAPE, len(mats), RESOLVE_SHAPE[1])
        ctx.set_materials(mats, texs)
        resolve_cases.device_resolve(ctx, attrs, ids, N.PBR_FILTER_POINT)
        result["resolve"] = report(ctx.debug_bounds(reset=True))
    np.savez(out_path, **result)
    print("front end under", N.LIB_PATH, {k: dict(zip(CLASSES, v.tolist())) for k, v in result.items()}, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
