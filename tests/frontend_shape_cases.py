"""Shapes and inputs of tests/test_gpu_frontend_shapes.py and tests/test_frontend_shapes_host.py: the frames at which
every front-end entry point is run beside the usual 70x37 and 256x64 -- an odd width of more than one 64-wide tile, a
lone column in a second tile, the tile's last column missing, and frames of one pixel, one column and one row -- the two
row strides of each, and the resolve inputs whose last column can tell a kernel that invents an x partner from one that
does not ("a partner is valid iff it lies inside the call's width and height"). A helper, not a test.
Run as a script (under whatever library PBR_LIB_PATH names -- the bounds-checked build, in a fresh child process) it
writes the device results of BOUNDS cases and the bounds flags to the .npz given."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resolve_aniso_cases as AC  # noqa: E402
import resolve_cases as C  # noqa: E402
import resolve_mip_cases as MC  # noqa: E402

F = np.float32

# (W, H). 71x37: two tiles in x, five in y, odd both ways. 63x5 / 65x2: the tile's last column missing / a lone column
# in a second tile. 1x1, 1x9, 3x1: every quad partner in x, in y or in both is outside the frame.
ODD_FRAMES = ((71, 37), (63, 5), (65, 2), (1, 1), (1, 9), (3, 1))
BIG, SMALL = ODD_FRAMES[0], ODD_FRAMES[1:]


def frame_id(frame):
    return f"{frame[0]}x{frame[1]}"


def strides(W):
    """The two row strides of a W-wide frame: an odd one (the scalar accesses) and the next even number above W (the
    paired accesses; with an odd W the last column is a pair's first half and takes the scalar tail)."""
    return (W if W % 2 else W + 1, W + 1 if W % 2 else W + 2)


# The raster cases run at every small frame (all of raster_cases.CASES run at 71x37).
SMALL_RASTER_CASES = ("one_triangle", "offscreen", "fan", "uv_sphere", "nan_inf")
CLIP_CASES = ("floor_grid", "inside_sphere", "single_n1_rot1_cull1_back", "single_n2_rot2_cull0_front")
ALPHA_CASES = ("checker_small", "clip_floor_sphere", "mixed")
LAYER_CASES = ("intersecting", "clipped_pane", "nested_mixed")
FLAG_FRAMES = ((71, 37), (65, 2))
UNEVEN_BANDS = ((0, 5), (5, 6), (6, 28), (28, 37))  # of a 37-row frame, as tests/test_gpu_raster.py cuts its own

# ---- resolve inputs ---------------------------------------------------------------------------------------------------

ALL_FLAGS = 7  # MC.table(): every flag, every map another size
# Ramps in texels of a 64-wide map per pixel in x (1 texel per pixel in y), and the materials they run under: diffuse
# alone over the 64x64 and the 256x1 chain textures, and the material whose every map has another size.
RAMP_TEXELS = (2, 8)
RAMP_MATERIALS = (13, 15, ALL_FLAGS)
BIASES = (0.0, 1.5)
ANISOTROPIES = (1, 8, 16)
# Odd-height bands of the 37-row frame; the first two end inside the frame: there the last row's y partner is outside
# the call's height ("Bands"), though the row below exists in memory with the same id.
INNER_BANDS = ((0, 5), (6, 13))
LAST_BAND = (12, 37)


def ramp_case(h, w, texels, material):
    """(attrs, ids): u = 0.125 + x * texels / 64, v = -0.5 + y / 64 under one material."""
    attrs = MC.ramp_attributes(h, w, texels / 64.0, 1.0 / 64.0, u0=0.125, v0=-0.5)
    return attrs, np.full((h, w), material, np.uint16)


def band_cases(h, w):
    """{name: (attrs, ids)} of the inputs the odd-height bands run: a ramp of 1 texel per pixel in x and 4 in y (the
    level comes from y, so a last row without its y partner takes another level than the same row in the full frame)
    and the per-quad footprints."""
    attrs = MC.ramp_attributes(h, w, 1.0 / 64.0, 4.0 / 64.0, u0=0.125, v0=-0.5)
    return {"y_ramp": (attrs, np.full((h, w), ALL_FLAGS, np.uint16)), "quads": quads_case(h, w)}


def special_case(h, w, n_materials):
    """The special UVs with a material per 2 x 2 quad (valid partners), as resolve_mip_cases.special_attributes."""
    return MC.special_attributes(h, w, n_materials, seed=w + 2 * h)


def quads_case(h, w):
    """Per-quad footprints under a material per quad: tap counts 1 .. 16 side by side."""
    return AC.quad_attributes(h, w, seed=w + 3), AC.quad_ids(h, w, AC.TEXTURED, seed=w + 4)


def widened(attrs, ids):
    """The frame one column wider: the column resolve_cases.padded_inputs(pad=True) puts behind the last one."""
    w = attrs.shape[2]
    a, i = C.padded_inputs(attrs, ids, w + 1, pad=True)
    return np.ascontiguousarray(a), np.ascontiguousarray(i)


def last_column_tells(want, want_wide):
    """Whether a result's last column differs, in some plane on some row, from its own column W - 2 or from the same
    column of the result on the widened frame: the conditions under which a kernel that invented the x partner of an
    odd width's last column could not pass."""
    planes, wide = want[0], want_wide[0]
    w = planes.shape[2]
    own = w >= 2 and bool((planes[:, :, w - 1].view(np.uint32) != planes[:, :, w - 2].view(np.uint32)).any())
    other = bool((planes[:, :, w - 1].view(np.uint32) != wide[:, :, w - 1].view(np.uint32)).any())
    return own, other


# ---- the bounds-checked build -----------------------------------------------------------------------------------------

def bounds_cases():
    """(mats, texs, [(name, call, attrs, ids, max_anisotropy, lod_bias, stride)]): one odd-width trilinear and one
    odd-width anisotropic case in both strides, the padding columns valid-looking."""
    mats, texs = MC.table()
    h, w = BIG[1], BIG[0]
    attrs, ids = ramp_case(h, w, 8, ALL_FLAGS)
    qa, qi = quads_case(5, w)
    return mats, texs, [("mip_71", "mip", attrs, ids, 0, 0.0, w), ("mip_72", "mip", attrs, ids, 0, 1.5, w + 1),
                        ("aniso_71", "aniso", qa, qi, 16, 0.0, w), ("aniso_72", "aniso", qa, qi, 8, 0.25, w + 1)]


def main(out_path):
    """bounds_cases() under the loaded library; the bounds flags of a bounds-checked build."""
    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd.renderer import ShadingContext

    mats, texs, cases = bounds_cases()
    result = {}
    with ShadingContext(0) as ctx:
        ctx.set_materials(mats, texs)
        ctx.generate_mips()
        for name, call, attrs, ids, m, bias, stride in cases:
            if call == "mip":
                planes, opacity, cov = MC.device_resolve_mip(ctx, attrs, ids, bias, stride, pad=True)
            else:
                planes, opacity, cov = AC.device_resolve_aniso(ctx, attrs, ids, m, bias, stride, pad=True)
            result[name + "__planes"], result[name + "__opacity"], result[name + "__coverage"] = planes, opacity, cov
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("odd-width resolves under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
