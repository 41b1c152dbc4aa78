"""Inputs of tests/test_raster_layer_host.py and tests/test_gpu_raster_layer.py: scenes of transparent draws over an
optional opaque layer (pbr_rasterize_layer), in the two frames of tests/raster_cases.py, and the
helpers that run a layer, and a whole peel, on the device. A helper, not a test. Run as a script (BOUNDS_CASES under
whatever library PBR_LIB_PATH names -- the bounds-checked build, in a fresh child process, as tests/raster_cases.py
does) it writes the device results and the bounds flags to the .npz given.

Most scenes are quads in pixel coordinates under raster_cases.PERSP, where a vertex's w picks its depth (larger w =
farther). A case is (meshes, opaque draws, transparent draws, view, clip_near): the opaque draws give the incoming
depth d_0 (1 where they draw nothing), the transparent draws are peeled against it."""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import raster_alpha_cases as AC  # noqa: E402
import raster_cases as C  # noqa: E402
import raster_clip_cases as CC  # noqa: E402
from physically_based_renderer_amd import _native as N  # noqa: E402
from physically_based_renderer_amd import scenes as S  # noqa: E402
from physically_based_renderer_amd.renderer import Draw  # noqa: E402

FRAMES = C.FRAMES
Scene = namedtuple("Scene", "meshes opaque draws view clip_near")


def nested(W, H, ws, seed, nx=1, ny=1):
    """len(ws) nested quads, quad k at PosH.w = ws[k], each a little smaller than the one before."""
    return [AC.px_grid(W, H, 2.25 + 3 * k, 1.5 + 2 * k, W - 3.5 - 3 * k, H - 2.25 - 2 * k, w, nx, ny, seed=seed + k)
            for k, w in enumerate(ws)]


def tilted(W, H, w_left, w_right, seed):
    """A quad over most of the frame whose depth runs from w_left at its left edge to w_right at its right edge."""
    m = AC.px_grid(W, H, 3.25, 2.5, W - 4.5, H - 3.25, 1.0, seed=seed)
    pts = [(3.25, 2.5, w_left), (W - 4.5, 2.5, w_right), (3.25, H - 3.25, w_left), (W - 4.5, H - 3.25, w_right)]
    m.vertices[:, 0:3] = C.px_vertices(pts, W, H, seed)[:, 0:3]
    return m


def case(name, W, H):
    view = C.screen_view(W, H)
    clip_near, opaque = False, []
    if name in ("nested_far_near", "nested_near_far", "nested_mixed"):  # chains of 3, 1 and 3
        ws = {"nested_far_near": (3.0, 2.0, 1.0), "nested_near_far": (1.0, 2.0, 3.0),
              "nested_mixed": (2.0, 3.0, 1.0, 2.5, 0.8)}[name]
        m = nested(W, H, ws, 100)
        d = [Draw(mesh=k, material=k, cull=1) for k in range(len(ws))]
    elif name == "equal_z":  # z = +0 everywhere: the second and third quad tie with the first and are not accepted
        view = C.screen_view(W, H, C.FLAT)
        m = nested(W, H, (1.0, 1.0, 2.0), 110)
        d = [Draw(mesh=k, material=k, cull=1) for k in range(3)]
    elif name == "intersecting":  # two quads that cross in the middle of the frame, and a third behind both
        m = [tilted(W, H, 1.0, 3.0, 120), tilted(W, H, 3.0, 1.0, 121),
             AC.px_grid(W, H, 6.0, 4.0, W - 9.0, H - 6.5, 4.0, seed=122)]
        d = [Draw(mesh=2, material=2, cull=1), Draw(mesh=0, material=0, cull=1), Draw(mesh=1, material=1, cull=1)]
    elif name == "sphere":  # a cull-none sphere overlapping itself: front and back faces in index order
        view = S.look_at_view((0.4, 0.3, -3.0), (0.0, 0.1, 0.0), np.pi / 3, W, H)
        m = [S.uv_sphere(16, 8)]
        d = [Draw(mesh=0, material=4, cull=1), Draw(mesh=0, material=5, cull=1, world=S.translation(0.5, 0.1, 0.8))]
    elif name == "clipped_pane":  # a pane from in front of the eye to behind it, a floor under the eye, a sphere
        view, clip_near = CC.camera(W, H), True
        pane = CC.soup([(-0.6, -0.9, -4.0), (-0.6, 0.9, -4.0), (0.5, 0.9, 3.0),
                        (-0.6, -0.9, -4.0), (0.5, 0.9, 3.0), (0.5, -0.9, 3.0)], 130)
        m = [CC.floor(3, 4), pane, S.uv_sphere(12, 6)]
        opaque = [Draw(mesh=2, material=3, world=S.translation(0.3, -0.2, 2.0))]
        d = [Draw(mesh=0, material=0, cull=1), Draw(mesh=1, material=1, cull=1),
             Draw(mesh=2, material=2, cull=1, world=S.translation(-0.4, -0.5, 0.5))]
    elif name == "small_triangles":  # every triangle's box <= 64 pixels: the setup lanes' loop, three deep
        nx, ny = -(-W // 7), -(-H // 7)
        m = nested(W, H, (3.0, 2.0, 1.0), 140, nx, ny)
        d = [Draw(mesh=k, material=k, cull=1) for k in range(3)]
    elif name == "larger_than_frame":  # triangles larger than the frame, far to near, and a quad between them
        m = [C.soup([(-W, -H, 3), (3 * W, -H, 3), (-W, 3 * H, 3), (-2 * W, -H, 1), (2 * W, -H, 1), (W // 2, 4 * H, 1)],
                    W, H, 150), AC.px_grid(W, H, 5.5, 3.25, W - 7.0, H - 5.0, 2.0, seed=151)]
        d = [Draw(mesh=0, material=0, cull=1, first_index=0, index_count=3), Draw(mesh=1, material=1, cull=1),
             Draw(mesh=0, material=2, cull=1, first_index=3, index_count=3)]
    elif name in ("panes_background", "panes_opaque"):  # panes at w = 3, 1.5, 1; the opaque quad at w = 2
        m = nested(W, H, (3.0, 1.5, 1.0), 160) + [AC.behind(W, H)]
        d = [Draw(mesh=k, material=k, cull=1) for k in range(3)]
        if name == "panes_opaque":  # the far pane is hidden where the opaque quad is, the near panes are not
            opaque = [Draw(mesh=3, material=7)]
    else:
        raise KeyError(name)
    return Scene(m, opaque, d, view, clip_near)


# name -> the longest chain of accepted fragments at a pixel, from the submission order (None: not fixed by hand).
# nested_mixed: w = 2, 3, 1, 2.5, 0.8 in that order: the strict running minima are 2, 1 and 0.8. intersecting: the far
# quad, then the quad nearer on the left, then on the right half the quad nearer there.
CHAINS = {"nested_far_near": 3, "nested_near_far": 1, "nested_mixed": 3, "equal_z": 1, "intersecting": 3,
          "sphere": None, "clipped_pane": None, "small_triangles": 3, "larger_than_frame": 3, "panes_background": 3,
          "panes_opaque": 3}
CASES = tuple(CHAINS)


def device_depth0(ctx, sc, stride, stream=None):
    """The opaque layer's depth plane on the device, (H, stride) float32 (1 where nothing is drawn): pbr_rasterize[_flags]
    of the opaque draws."""
    import torch

    from physically_based_renderer_amd.renderer import Attributes

    dev = torch.device("cuda", 0)
    W, H = sc.view.width, sc.view.height
    planes = torch.empty((14, H, stride), dtype=torch.float32, device=dev)
    ids = torch.empty((H, stride), dtype=torch.int16, device=dev)
    depth = torch.full((H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
    ctx.rasterize(sc.opaque, sc.view, out=(Attributes(planes, ids, width=W), depth), stream=stream,
                  clip_near=sc.clip_near)
    return depth


def device_layer(ctx, sc, depth_in, prim_in, stride=None, rows=None, alias=False, stream=None):
    """One pbr_rasterize_layer into sentinel-filled canvases (or, with ``alias``, with the depth plane being
    ``depth_in`` and prim_out being ``prim_in``, which must then be given); ``depth_in`` and ``prim_in`` are (H, stride)
    device tensors. Returns (planes, ids, depth, prim) as device tensors and the four counter dicts, synchronised."""
    import torch

    from physically_based_renderer_amd.renderer import Attributes

    dev = torch.device("cuda", 0)
    W, H = sc.view.width, sc.view.height
    stride = W + 1 if stride is None else stride
    planes = torch.full((14, H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
    ids = torch.full((H, stride), C.SENTINEL_ID, dtype=torch.int16, device=dev)
    depth = depth_in if alias else torch.full((H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
    prim = prim_in if alias else torch.full((H, stride), C.SENTINEL_ID, dtype=torch.int32, device=dev)
    flags = N.PBR_RASTER_CLIP_NEAR if sc.clip_near else 0
    r0, r1 = (0, H) if rows is None else rows
    view = sc.view if rows is None else sc.view.rows(r0, r1)
    ctx.rasterize_layer(sc.draws, view, depth_in[r0:r1], None if prim_in is None else prim_in[r0:r1], flags,
                        out=(Attributes(planes[:, r0:r1], ids[r0:r1], width=W), depth[r0:r1]), prim_out=prim[r0:r1],
                        stream=stream)
    counters = (ctx.raster_stats(stream=stream), ctx.raster_clip_stats(stream=stream),
                ctx.raster_layer_stats(stream=stream), ctx.raster_alpha_stats(stream=stream))
    torch.cuda.synchronize()
    return (planes, ids, depth, prim), counters


def to_host(tensors):
    planes, ids, depth, prim = tensors
    return (planes.cpu().numpy(), ids.cpu().numpy().view(np.uint16), depth.cpu().numpy(),
            prim.cpu().numpy().view(np.uint32))


def padded(a, stride, fill):
    """A (rows, W) host plane as an (rows, stride) device tensor, the padding columns holding ``fill``."""
    import torch

    out = np.full((a.shape[0], stride), fill, a.dtype)
    out[:, :a.shape[1]] = a
    if a.dtype == np.uint32:
        out = out.view(np.int32)
    return torch.from_numpy(out).to(torch.device("cuda", 0))


BOUNDS_CASES = (("small_triangles", "70x37"), ("larger_than_frame", "256x64"), ("clipped_pane", "70x37"))


def main(out_path):
    """BOUNDS_CASES peeled (separate planes, odd stride) under the loaded library; the bounds flags of a
    bounds-checked build. Layer k of a case is stored under <case>_<frame>__<k>__..."""
    import torch

    from physically_based_renderer_amd.renderer import ShadingContext

    result = {}
    with ShadingContext(0) as ctx:
        for name, frame in BOUNDS_CASES:
            W, H = FRAMES[frame]
            sc = case(name, W, H)
            ctx.set_meshes(sc.meshes)
            depth, prim = device_depth0(ctx, sc, W + 1), None
            key = f"{name}_{frame}"
            for k in range(16):
                got, (stats, clip, layer, _) = device_layer(ctx, sc, depth, prim)
                planes, ids, depth_k, prim_k = to_host(got)
                result[f"{key}__{k}__planes"], result[f"{key}__{k}__ids"] = planes, ids
                result[f"{key}__{k}__depth"], result[f"{key}__{k}__prim"] = depth_k, prim_k
                result[f"{key}__{k}__stats"] = np.array([stats[s] for s in sorted(stats)] +
                                                        [clip[s] for s in sorted(clip)] +
                                                        [layer[s] for s in sorted(layer)], np.int64)
                if layer["layer_fragments"] == 0:
                    break
                depth, prim = got[2], got[3]
            result[key + "__layers"] = np.array(k + 1)
        torch.cuda.synchronize()
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds", "raster", "mesh")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")  # the raster kernels' unit
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("layers under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
