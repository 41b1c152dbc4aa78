"""Inputs of tests/test_raster_alpha_host.py and tests/test_gpu_raster_alpha.py: scenes with alpha-tested materials
(pbr_rasterize_flags with PBR_RASTER_ALPHA_TEST), in the two frames of tests/raster_cases.py, and
the helper that runs one on the device. A helper, not a test. Run as a script (BOUNDS_CASES under whatever library
PBR_LIB_PATH names -- the bounds-checked build, in a fresh child process, as tests/raster_cases.py does) it writes the
device results and the bounds flags to the .npz given.

Most scenes are quads in pixel coordinates under raster_cases.PERSP (a vertex's w picks its depth): a tested quad at
w = 1 in front of an opaque quad at w = 2 that covers part of the frame, so a discarded fragment shows the opaque quad in
some pixels and the background in others. Material ids: what each case says; OPAQUE is the id of the untested material
behind."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import raster_cases as C  # noqa: E402
import raster_clip_cases as CC  # noqa: E402
from physically_based_renderer_amd import _native as N  # noqa: E402
from physically_based_renderer_amd import scenes as S  # noqa: E402
from physically_based_renderer_amd.renderer import Draw, Material, Mesh  # noqa: E402

FRAMES = C.FRAMES
ALPHA = N.PBR_MAT_ALPHA_TEST


def tested(tex_index):
    """A material whose opacity comes from texture `tex_index` under the alpha test."""
    return Material(diffuse_albedo=(0.2, 0.7, 0.3), roughness=0.6, flags=ALPHA, tex=(-1, -1, -1, -1, -1, tex_index))


def opaque(opacity=1.0):
    return Material(diffuse_albedo=(0.6, 0.5, 0.4), roughness=0.8, opacity=opacity)


def with_channels(red, channels):
    """An (h, w, channels) texture with `red` in .r; green and blue hold its complement, alpha a third pattern: a
    test that read another byte would decide otherwise."""
    red = np.asarray(red, np.uint8)
    if channels == 1:
        return red[:, :, None].copy()
    t = np.empty(red.shape + (channels,), np.uint8)
    t[..., 0], t[..., 1], t[..., 2] = red, 255 - red, 255 - red
    if channels == 4:
        t[..., 3] = 255 - red
    return t


def checker(w, h, channels=1, invert=False):
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return with_channels(np.where(((i + j) % 2 == 0) != invert, 255, 0), channels)


def around_threshold(w, h, seed, channels=1):
    """Random bytes, half of them within a few steps of the threshold 25 | 26."""
    rng = np.random.default_rng(seed)
    near = rng.integers(20, 32, (h, w))
    far = rng.integers(0, 256, (h, w))
    return with_channels(np.where(rng.random((h, w)) < 0.5, near, far), channels)


def px_grid(W, H, x0, y0, x1, y1, w, nx=1, ny=1, uv0=(0.0, 0.0), uv1=(1.0, 1.0), seed=0, back=False):
    """An nx x ny grid of quads with shared vertices over the pixel rectangle [x0, x1] x [y0, y1] at PosH.w = `w`,
    clockwise on the screen (front faces; `back`: counter-clockwise), uv from uv0 to uv1, random other attributes."""
    j, i = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    fx, fy = (i / nx).ravel(), (j / ny).ravel()
    pts = np.stack([x0 + (x1 - x0) * fx, y0 + (y1 - y0) * fy, np.full(fx.shape, float(w))], -1)
    v = C.px_vertices(pts, W, H, seed)
    v[:, 12] = uv0[0] + (uv1[0] - uv0[0]) * fx
    v[:, 13] = uv0[1] + (uv1[1] - uv0[1]) * fy
    ring = nx + 1
    tris = []
    for r in range(ny):
        for c in range(nx):
            v00, v01, v10, v11 = r * ring + c, r * ring + c + 1, (r + 1) * ring + c, (r + 1) * ring + c + 1
            tris += [(v00, v11, v01), (v00, v10, v11)] if back else [(v00, v01, v11), (v00, v11, v10)]
    return Mesh(v, np.array(tris, np.uint32).reshape(-1))


def behind(W, H):
    """The opaque quad at w = 2 over the right two thirds of the frame and all but its top rows."""
    return px_grid(W, H, W // 3 + 0.25, 3.5, W - 1.5, H - 0.75, 2.0, seed=90)


def matrix(rows):
    return tuple(np.asarray(rows, np.float32).ravel().tolist())


def scale_translate(su, sv, tu, tv):
    return matrix([[su, 0, 0, 0], [0, sv, 0, 0], [0, 0, 1, 0], [tu, tv, 0, 1]])


def case(name, W, H):
    """(meshes, draws, view, materials, textures, clip_near) of one named case in a W x H frame."""
    view = C.screen_view(W, H)
    clip_near = False
    front = (2.25, 1.5, W - 3.5, H - 2.25)  # the tested quad's rectangle in most cases
    if name in ("checker_large", "checker_small"):  # 1: two large triangles; every triangle's box <= 64 pixels
        nx, ny = (1, 1) if name == "checker_large" else (-(-W // 7), -(-H // 7))
        m = [px_grid(W, H, *front, 1.0, nx, ny, seed=31), behind(W, H)]
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=1)]
        mats, texs = [tested(0), opaque()], [checker(4, 4)]
    elif name == "threshold":  # 2: every byte 0..255, a texel per pixel: pixel centres on texel centres
        m = [px_grid(W, H, 3.0, 2.0, 19.0, 18.0, 1.0, seed=32), px_grid(W, H, 1.5, 8.25, 40.0, 30.0, 2.0, seed=33)]
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=1)]
        mats, texs = [tested(0), opaque()], [with_channels(np.arange(256).reshape(16, 16), 3)]
    elif name in ("sizes_c1", "sizes_c3", "sizes_c4"):  # 3: 1x1 (one discards, one keeps), 5x3 and 64x64 textures
        ch = int(name[-1])
        texs = [with_channels([[7]], ch), with_channels([[26]], ch), around_threshold(5, 3, 41 + ch, ch),
                around_threshold(64, 64, 51 + ch, ch)]
        mats = [tested(k) for k in range(4)] + [opaque()]
        q = (W - 4) / 4.0
        m = [px_grid(W, H, 2.25 + k * q, 1.5, 1.75 + (k + 1) * q, H - 2.25, 1.0, seed=34 + k) for k in range(4)]
        m.append(behind(W, H))
        d = [Draw(mesh=k, material=k) for k in range(4)] + [Draw(mesh=4, material=4)]
    elif name == "wrap":  # 4: uv in [-3.6, 3.9] x [1.75, -2.75] through both transforms
        m = [px_grid(W, H, *front, 1.0, seed=35), behind(W, H)]
        d = [Draw(mesh=0, material=0, tex_transform=scale_translate(3.0, -1.5, -1.25, 0.5),
                  mat_transform=scale_translate(2.5, 3.0, -0.475, 0.25)), Draw(mesh=1, material=1)]
        mats, texs = [tested(0), opaque()], [around_threshold(5, 3, 36, 3)]
    elif name == "nan_transform":  # 5: a NaN entry reaches u and v (0 * NaN): texel 0 of each texture decides
        t = np.eye(4, dtype=np.float32)
        t[0, 0] = np.nan
        half = (W - 4) / 2.0
        m = [px_grid(W, H, 2.25, 1.5, 2.0 + half, H - 2.25, 1.0, seed=37),
             px_grid(W, H, 2.5 + half, 1.5, W - 3.5, H - 2.25, 1.0, seed=38), behind(W, H)]
        d = [Draw(mesh=0, material=0, tex_transform=matrix(t)), Draw(mesh=1, material=1, tex_transform=matrix(t)),
             Draw(mesh=2, material=2)]
        zero_first, full_first = np.full((4, 4), 255), np.zeros((4, 4))
        zero_first[0, 0], full_first[0, 0] = 0, 255
        mats, texs = [tested(0), tested(1), opaque()], [with_channels(zero_first, 1), with_channels(full_first, 1)]
    elif name == "texel_edges":  # 6: a pixel per texel, shifted half a texel: every uv lands on a texel edge
        m = [px_grid(W, H, 5.0, 3.0, 37.0, 19.0, 1.0, seed=39), behind(W, H)]
        d = [Draw(mesh=0, material=0, mat_transform=scale_translate(1.0, 1.0, 0.5 / 32.0, 0.5 / 16.0)),
             Draw(mesh=1, material=1)]
        mats, texs = [tested(0), opaque()], [checker(32, 16, 4)]
    elif name == "complementary":  # 7: equal depth everywhere (z = +0): the later draw wins where the earlier is cut
        view = C.screen_view(W, H, C.FLAT)
        m = [px_grid(W, H, *front, 1.0, seed=40)]
        d = [Draw(mesh=0, material=0), Draw(mesh=0, material=1)]
        mats, texs = [tested(0), tested(1)], [checker(6, 4), checker(6, 4, invert=True)]
    elif name == "cull_none_back":  # 8: counter-clockwise under cull none: setup exchanges vertices 1 and 2
        m = [px_grid(W, H, *front, 1.0, 2, 1, seed=42, back=True), behind(W, H)]
        d = [Draw(mesh=0, material=0, cull=1), Draw(mesh=1, material=1)]
        mats, texs = [tested(0), opaque()], [around_threshold(5, 3, 43, 4)]
    elif name == "cull_back":  # 9: the counter-clockwise half is culled, the clockwise half tested
        half = W / 2.0
        m = [px_grid(W, H, 2.25, 1.5, half, H - 2.25, 1.0, seed=44, back=True),
             px_grid(W, H, half, 1.5, W - 3.5, H - 2.25, 1.0, seed=45), behind(W, H)]
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=0), Draw(mesh=2, material=1)]
        mats, texs = [tested(0), opaque()], [checker(8, 4, 3)]
    elif name == "mixed":  # 10: tested, untested, an id past the table, an untested material with opacity 0
        q = (W - 4) / 4.0
        m = [px_grid(W, H, 2.25 + k * q, 1.5, 1.75 + (k + 1) * q, H - 2.25, 1.0, seed=46 + k) for k in range(4)]
        m.append(behind(W, H))
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=1), Draw(mesh=2, material=7), Draw(mesh=3, material=2),
             Draw(mesh=4, material=1)]
        mats, texs = [tested(0), opaque(), opaque(0.0)], [checker(4, 4, 3)]
    elif name == "clip_floor_sphere":  # 11: a tested floor under the eye, a tested sphere around it, opaque spheres
        view, clip_near = CC.camera(W, H), True
        big = np.diag([3.0, 3.0, 3.0, 1.0]).astype(np.float32)
        m = [CC.floor(3, 4), S.uv_sphere(12, 6)]
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=1, cull=1, world=matrix(big)),
             Draw(mesh=1, material=2, world=S.translation(0.3, -0.7, 1.0)),
             Draw(mesh=1, material=3, world=S.translation(-1.2, 0.1, 0.5))]
        mats = [tested(0), tested(1), opaque(), Material(diffuse_albedo=(0.95, 0.64, 0.54), metallic=1.0, roughness=0.35)]
        texs = [checker(6, 14, 3), checker(16, 8, 1)]
    elif name == "all_zero":  # 12: every fragment discarded: the frame is the background
        m = [px_grid(W, H, *front, 1.0, seed=50), px_grid(W, H, 4.5, 3.25, W - 8.0, H - 4.0, 2.0, 5, 3, seed=51)]
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=0, cull=1)]
        mats, texs = [tested(0)], [with_channels(np.zeros((3, 2)), 4)]
    elif name == "all_255":  # 13: nothing discarded
        m = [px_grid(W, H, *front, 1.0, seed=52), behind(W, H)]
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=1)]
        mats, texs = [tested(0), opaque()], [with_channels(np.full((3, 2), 255), 3)]
    elif name == "no_tested":  # 13: the flag with no tested material (opacity 0 is not a test)
        m = [px_grid(W, H, *front, 1.0, 3, 2, seed=53), behind(W, H)]
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=1), Draw(mesh=1, material=9)]
        mats, texs = [opaque(0.0), opaque()], [checker(4, 4)]
    else:
        raise KeyError(name)
    return m, d, view, mats, texs, clip_near


# The cases every one of which discards some fragments and keeps others, and those that discard all or none.
CUTOUT_CASES = ("checker_large", "checker_small", "threshold", "sizes_c1", "sizes_c3", "sizes_c4", "wrap",
                "nan_transform", "texel_edges", "complementary", "cull_none_back", "cull_back", "mixed",
                "clip_floor_sphere")
CASES = CUTOUT_CASES + ("all_zero", "all_255", "no_tested")


def device_rasterize(ctx, meshes, draws, view, materials, textures, clip_near=False, alpha_test=True, stride=None,
                     rows=None, stream=None, upload=True):
    """Rasterise through pbr_rasterize_flags with PBR_RASTER_ALPHA_TEST (and PBR_RASTER_CLIP_NEAR) into
    sentinel-filled canvases; returns (planes, material, depth, stats, clip stats, alpha stats), synchronised."""
    import torch

    from physically_based_renderer_amd.renderer import Attributes

    flags = (N.PBR_RASTER_CLIP_NEAR if clip_near else 0) | (N.PBR_RASTER_ALPHA_TEST if alpha_test else 0)
    dev = torch.device("cuda", 0)
    W, H = view.width, view.height
    stride = W + 1 if stride is None else stride
    planes = torch.full((14, H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
    ids = torch.full((H, stride), C.SENTINEL_ID, dtype=torch.int16, device=dev)
    depth = torch.full((H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
    if upload:
        ctx.set_meshes(meshes, stream=stream)
        ctx.set_materials(materials, textures, stream=stream)
    torch.cuda.synchronize()
    if rows is None:
        ctx.rasterize_flags(draws, view, flags, out=(Attributes(planes, ids, width=W), depth), stream=stream)
    else:
        r0, r1 = rows
        ctx.rasterize_flags(draws, view.rows(r0, r1), flags,
                            out=(Attributes(planes[:, r0:r1], ids[r0:r1], width=W), depth[r0:r1]), stream=stream)
    stats, clip = ctx.raster_stats(stream=stream), ctx.raster_clip_stats(stream=stream)
    alpha = ctx.raster_alpha_stats(stream=stream)
    torch.cuda.synchronize()
    return planes.cpu().numpy(), ids.cpu().numpy().view(np.uint16), depth.cpu().numpy(), stats, clip, alpha


BOUNDS_CASES = (("checker_small", "70x37"), ("wrap", "256x64"), ("nan_transform", "70x37"),
                ("clip_floor_sphere", "256x64"))


def main(out_path):
    """BOUNDS_CASES, flagged, under the loaded library; the bounds flags of a bounds-checked build."""
    from physically_based_renderer_amd.renderer import ShadingContext

    result = {}
    with ShadingContext(0) as ctx:
        for name, frame in BOUNDS_CASES:
            W, H = FRAMES[frame]
            planes, ids, depth, stats, clip, alpha = device_rasterize(ctx, *case(name, W, H))
            key = f"{name}_{frame}"
            result[key + "__planes"], result[key + "__ids"], result[key + "__depth"] = planes, ids, depth
            result[key + "__stats"] = np.array([stats[k] for k in sorted(stats)] + [clip[k] for k in sorted(clip)] +
                                               [alpha[k] for k in sorted(alpha)], np.int64)
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds", "raster", "mesh")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")  # the raster kernels' unit
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("alpha-tested rasterize under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
