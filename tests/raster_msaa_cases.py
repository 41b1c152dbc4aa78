"""Inputs of tests/test_raster_msaa_host.py and tests/test_gpu_raster_msaa.py: small scenes in pixel coordinates that
walk the rules of four samples per pixel, the smallest that can still go wrong, and the helper
that runs one on the device. A helper, not a test. Run as a script (a few cases under whatever library PBR_LIB_PATH
names -- the bounds-checked build, in a fresh child process, as tests/raster_cases.py does) it writes the device results
and the bounds flags to the .npz given.

Sample s of pixel (x, y) is at (x + 0.5 + dx / 16, y + 0.5 + dy / 16) px with (dx, dy) = raster_msaa_reference.OFFSETS."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import raster_cases as C  # noqa: E402
from raster_msaa_reference import OFFSETS  # noqa: E402
from physically_based_renderer_amd.renderer import Draw  # noqa: E402

FRAMES = C.FRAMES
VIS_SENTINEL = 0x0123456789ABCDEF
OWNER_SENTINEL = 0xA5


def sample_px(x, y, s):
    """Sample s of pixel (x, y) in pixels."""
    return x + 0.5 + OFFSETS[s][0] / 16.0, y + 0.5 + OFFSETS[s][1] / 16.0


def around(px, py, r, w=1.0):
    """A triangle of 'radius' r px around the point (px, py), on the 1/256 grid."""
    q = lambda f: np.floor(f * 256) / 256  # noqa: E731
    return [(q(px - r), q(py - 0.6 * r), w), (q(px + r), q(py - 0.5 * r), w), (q(px + 0.1 * r), q(py + r), w)]


def case(name, W, H):
    """(meshes, draws, view) of one named case in a W x H frame."""
    view = C.screen_view(W, H)
    if name == "one_sample_no_centre":  # covers sample 1 of pixel (7, 5) and nothing else: no pixel centre at all
        m, d = C.one_draw(around(*sample_px(7, 5, 1), 0.1), W, H, 31, cull=1)
    elif name == "subpixel_each_sample":  # one sub-pixel triangle around each sample point of pixel (12, 9)
        pts = []
        for s in range(4):
            pts += around(*sample_px(12, 9, s), 0.09, 1.0 + 0.25 * s)
        m, d = C.one_draw(pts, W, H, 32, cull=1)
    elif name == "sliver":  # one sample wide, across the frame: every 64 x 4 block border and every band border
        m, d = C.one_draw([(1.2, 2.3, 1), (W - 1.6, H - 3.1, 2), (W - 1.6, H - 3.1 + 0.3, 2)], W, H, 33, cull=1)
    elif name == "box_boundary":
        # A: 8 x 8 pixels with reachable samples: the setup lane's last size. B: 8 x 8 pixel centres, 9 x 9 pixels with
        # reachable samples: listed for the large-triangle kernel although its centre box is small.
        m, d = C.one_draw([(10.9, 4.9, 1), (18.2, 5.5, 1), (14.0, 12.2, 1.5),
                           (30.4, 14.4, 1), (38.45, 15.0, 2), (33.0, 22.45, 1)], W, H, 34, cull=1)
    elif name == "larger_than_frame":
        m, d = C.one_draw([(-W, -H, 3), (3 * W, -H, 3), (-W, 3 * H, 1.5)], W, H, 35)
    elif name == "vertices_on_samples":  # every vertex exactly on a sample point
        a, b, c = sample_px(5, 4, 0), sample_px(30, 8, 1), sample_px(12, 25, 3)
        a2, b2, c2 = sample_px(40, 3, 2), sample_px(60, 20, 3), sample_px(41, 30, 0)
        m, d = C.one_draw([(*a, 1), (*b, 2), (*c, 1), (*a2, 1), (*b2, 1), (*c2, 1)], W, H, 36, cull=1)
    elif name in ("equal_depth_ab", "equal_depth_ba"):  # FLAT: every sample ties on depth, the earlier triangle wins
        m, d, view = C.case("coplanar_ab" if name.endswith("ab") else "coplanar_ba", W, H)
    elif name == "interpenetrating":  # a pixel's samples split by depth, not by an edge
        m, d, view = C.case("interpenetrating", W, H)
    elif name == "four_fragments":  # four triangles meet at the centre of pixel (20, 10): one sample each
        rim = [(10.5, 0.5), (30.5, 0.5), (30.5, 20.5), (10.5, 20.5)]
        m, d = C.one_draw(C.fan_points(20.5, 10.5, rim), W, H, 37, cull=1)
    elif name == "past_last_column_and_row":  # samples right of the last column and below the last row are not the frame's
        m, d = C.one_draw([(W - 0.3, 3.2, 1), (W + 2.5, 6.0, 1), (W - 0.2, 9.7, 1),
                           (4.1, H - 0.3, 1), (15.0, H - 0.25, 1), (9.0, H + 3.0, 2),
                           (W - 0.7, H - 0.7, 1), (W + 0.6, H - 0.5, 1), (W - 0.5, H + 0.8, 1)], W, H, 38, cull=1)
    elif name in ("reversed_cull_back", "reversed_cull_none", "near_and_guard", "uv_sphere", "random_subpixel",
                  "split_quad", "fan"):
        m, d, view = C.case(name, W, H)
    elif name == "large_tri":  # one triangle over most of the frame
        m, d = C.one_draw([(2.3, 1.7, 1), (W - 2.6, 3.1, 2), (W * 0.4, H - 1.4, 0.7)], W, H, 39)
    elif name == "zero_draws":
        m, d = C.one_draw([(2, 2, 1), (20, 4, 1), (8, 20, 1)], W, H, 40)
        d = []
    else:
        raise KeyError(name)
    return m, d, view


CASES = ("one_sample_no_centre", "subpixel_each_sample", "sliver", "box_boundary", "larger_than_frame",
         "vertices_on_samples", "equal_depth_ab", "equal_depth_ba", "interpenetrating", "four_fragments",
         "past_last_column_and_row", "reversed_cull_back", "reversed_cull_none", "near_and_guard", "uv_sphere",
         "random_subpixel", "large_tri", "zero_draws")


def device_msaa(ctx, meshes, draws, view, stride=None, rows=None, stream=None, set_meshes=True, slots=(0, 1, 2, 3)):
    """The whole sequence into sentinel-filled canvases with `stride` elements per row (default width + 1: odd for
    both frames): pbr_msaa_rasterize, then pbr_msaa_fragments for every slot of `slots`. Returns a dict: vis
    (4, band rows, stride) uint64, stats, and per slot k planes[k] (14, H, stride), ids[k], depth[k], owner[k]
    (H, stride) and msaa[k] (the slot counters after that call), synchronised. `rows` = (r0, r1): only that band, the
    targets through offset pointers into full canvases, the surface of the band's size."""
    import torch

    from physically_based_renderer_amd.renderer import Attributes

    dev = torch.device("cuda", 0)
    W, H = view.width, view.height
    stride = W + 1 if stride is None else stride
    r0, r1 = (0, H) if rows is None else rows
    v = view if rows is None else view.rows(r0, r1)
    surface = torch.full((4, r1 - r0, stride), VIS_SENTINEL, dtype=torch.int64, device=dev)
    if set_meshes:
        ctx.set_meshes(meshes, stream=stream)
    torch.cuda.synchronize()
    ctx.msaa_rasterize(draws, v, surface=surface, stream=stream)
    out = dict(stats=ctx.raster_stats(stream=stream), planes={}, ids={}, depth={}, owner={}, msaa={})
    for k in slots:
        planes = torch.full((14, H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
        ids = torch.full((H, stride), C.SENTINEL_ID, dtype=torch.int16, device=dev)
        depth = torch.full((H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
        owner = torch.full((H, stride), OWNER_SENTINEL, dtype=torch.uint8, device=dev)
        ctx.msaa_fragments(draws, v, surface, k, out=(Attributes(planes[:, r0:r1], ids[r0:r1], width=W), depth[r0:r1]),
                           owner=owner[r0:r1], stream=stream)
        out["msaa"][k] = ctx.msaa_stats(stream=stream)["slot_pixels"]
        out["planes"][k], out["ids"][k] = planes.cpu().numpy(), ids.cpu().numpy().view(np.uint16)
        out["depth"][k], out["owner"][k] = depth.cpu().numpy(), owner.cpu().numpy()
    out["stats_after"] = ctx.raster_stats(stream=stream)
    torch.cuda.synchronize()
    out["vis"] = surface.cpu().numpy().view(np.uint64)
    return out


BOUNDS_CASES = (("past_last_column_and_row", "70x37"), ("sliver", "256x64"), ("larger_than_frame", "70x37"),
                ("random_subpixel", "70x37"))


def main(out_path):
    """BOUNDS_CASES under the loaded library; the bounds flags of a bounds-checked build."""
    import torch

    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd.renderer import ShadingContext

    result = {}
    with ShadingContext(0) as ctx:
        for name, frame in BOUNDS_CASES:
            W, H = FRAMES[frame]
            m, d, v = case(name, W, H)
            got = device_msaa(ctx, m, d, v)
            key = f"{name}_{frame}"
            result[key + "__vis"] = got["vis"]
            result[key + "__stats"] = np.array([got["stats"][k] for k in sorted(got["stats"])], np.int64)
            for k in range(4):
                result[f"{key}__{k}__planes"], result[f"{key}__{k}__ids"] = got["planes"][k], got["ids"][k]
                result[f"{key}__{k}__depth"], result[f"{key}__{k}__owner"] = got["depth"][k], got["owner"][k]
                result[f"{key}__{k}__msaa"] = np.array(got["msaa"][k], np.int64)
        # the resolve under the same build: four slot frames, every owner byte
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(41)
        frames = rng.uniform(0, 2, (4, 5, 67, 4)).astype(np.float32)
        owner = rng.integers(0, 256, (5, 67)).astype(np.uint8)
        slots = [torch.from_numpy(f).to(dev) for f in frames]
        result["resolve__frames"], result["resolve__owner"] = frames, owner
        result["resolve__f32"] = ctx.msaa_resolve(slots, torch.from_numpy(owner).to(dev)).cpu().numpy()
        result["resolve__u8"] = ctx.msaa_resolve(slots, torch.from_numpy(owner).to(dev),
                                                 fmt=N.PBR_OUTPUT_RGBA8_UNORM).cpu().numpy()
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds", "raster", "mesh")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("msaa under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
