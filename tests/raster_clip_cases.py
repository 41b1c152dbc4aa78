"""Inputs of tests/test_raster_clip_host.py and tests/test_gpu_raster_clip.py: scenes with triangles across the near
plane, under a left-handed perspective camera (near 0.1, far 100; scenes.look_at_view), and
the helper that runs one on the device with PBR_RASTER_CLIP_NEAR. A helper, not a test. Run as a script (BOUNDS_CASES
under whatever library PBR_LIB_PATH names -- the bounds-checked build, in a fresh child process, as
tests/raster_cases.py does) it writes the device results and the bounds flags to the .npz given.

The camera of most scenes stands at EYE = (0, 0, -2) and looks along +z, so the near plane is z = -1.9: geometry with
z below that is in front of z = 0 in clip space ("outside"), i.e. beside or behind the eye."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import raster_cases as C  # noqa: E402
from physically_based_renderer_amd import scenes as S  # noqa: E402
from physically_based_renderer_amd.renderer import Draw, Mesh, View  # noqa: E402

FRAMES = C.FRAMES
EYE = (0.0, 0.0, -2.0)
FOV = np.pi / 3
FLOOR_Y = -1.0


def camera(W, H, eye=EYE, target=(0.0, 0.0, 1.0)):
    return S.look_at_view(eye, target, FOV, W, H)


def floor(nx, nz, x0=-3.0, x1=3.0, z0=-6.0, z1=8.0, y=FLOOR_Y):
    """An nx x nz grid of quads on the plane `y` with shared vertices, facing up (front faces seen from above):
    normal +y, tangent +x, bitangent +z, uv = the grid parameter."""
    j, i = np.meshgrid(np.arange(nz + 1), np.arange(nx + 1), indexing="ij")
    u, v = i / nx, j / nz
    n = (nx + 1) * (nz + 1)
    vert = np.zeros((n, 14), np.float32)
    vert[:, 0], vert[:, 1], vert[:, 2] = (x0 + (x1 - x0) * u).ravel(), y, (z0 + (z1 - z0) * v).ravel()
    vert[:, 4], vert[:, 6], vert[:, 11] = 1.0, 1.0, 1.0
    vert[:, 12], vert[:, 13] = u.ravel(), v.ravel()
    ring = nx + 1
    tris = []
    for r in range(nz):
        for c in range(nx):
            v00, v01, v10, v11 = r * ring + c, r * ring + c + 1, (r + 1) * ring + c, (r + 1) * ring + c + 1
            tris += [(v00, v10, v01), (v01, v10, v11)]
    return Mesh(vert, np.array(tris, np.uint32).reshape(-1))


def soup(points, seed):
    """A mesh of independent triangles over world-space points, random other attributes."""
    rng = np.random.default_rng(seed)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    v = rng.normal(size=(pts.shape[0], 14)).astype(np.float32)
    v[:, 0:3] = pts
    return Mesh(v, np.arange(v.shape[0], dtype=np.uint32))


# Case (c): one triangle with n inside vertices; vertex 0 of the base order is the odd one (the inside vertex of n = 1,
# the outside vertex of n = 2). Front-facing as listed (clockwise on the screen, y down); "back" exchanges 1 and 2.
SINGLE = {1: [(0.1, 0.2, 0.5), (1.4, -0.8, -4.0), (-1.2, -0.9, -3.5)],
          2: [(0.2, -0.6, -4.0), (-0.9, 0.5, 1.0), (1.1, 0.3, 0.5)]}
SINGLE_CASES = tuple(f"single_n{n}_rot{r}_cull{c}_{face}" for n in (1, 2) for r in (0, 1, 2) for c in (0, 1)
                     for face in ("front", "back"))

# Case (d): an orthographic-style ViewProj (w = 1) and a World whose zeros in the z column are -0.0f, so that for
# x, y > 0 every product of the z dot is -0.0f and a vertex with z = -0.0f keeps its sign down to PosH.z: (-0) + (-0)
# is -0, while one +0 term makes the sum +0.
ORTHO = np.array([[0.8, 0, -0.0, 0], [0, 0.8, -0.0, 0], [0, 0, 1.0, 0], [0, 0, -0.0, 1]], np.float32)
ORTHO_WORLD = np.array([[1, 0, -0.0, 0], [0, 1, -0.0, 0], [0, 0, 1, 0], [0, 0, -0.0, 1]], np.float32)


def case(name, W, H):
    """(meshes, draws, view) of one named case in a W x H frame."""
    view = camera(W, H)
    if name == "floor_quad":  # (a) two triangles from in front of the eye to behind it
        m, d = [floor(1, 1)], [Draw(mesh=0, material=1)]
    elif name == "floor_grid":  # (b) shared vertices: every crossing edge is cut by two triangles
        m, d = [floor(6, 6, z0=-4.0)], [Draw(mesh=0, material=2)]  # the row z in [-2, 0] crosses z = -1.9
    elif name.startswith("single_"):  # (c)
        _, n, rot, cull, face = name.split("_")
        p = list(SINGLE[int(n[1])])
        if face == "back":
            p[1], p[2] = p[2], p[1]
        r = int(rot[3])
        m, d = [soup([p[r % 3], p[(r + 1) % 3], p[(r + 2) % 3]], 21)], [Draw(mesh=0, material=3, cull=int(cull[4]))]
    elif name == "zero_z":  # (d) PosH.z exactly +0.0f and -0.0f (both inside) under an orthographic-style matrix
        view = View(view_proj=tuple(ORTHO.ravel().tolist()), width=W, height=H, eye=(0.5, -1.0, 2.0),
                    bg_right=(1.2, 0.0, 0.1), bg_up=(0.0, 0.7, 0.0), bg_forward=(0.1, 0.2, 1.0))
        m = [soup([(0.1, 0.1, 0.0), (1.1, 0.2, -0.5), (0.3, 1.0, 0.5),       # +0, outside, inside
                   (0.2, 0.3, -0.0), (0.9, 1.1, 0.25), (1.0, 0.1, -0.75),    # -0, inside, outside
                   (0.05, 0.6, 0.0), (0.5, 0.7, -0.0), (0.1, 1.15, 0.5),     # +0, -0, inside: not clipped
                   (0.6, 0.05, -0.0), (1.15, 0.4, -0.25), (0.7, 0.6, -0.5)], 22)]  # -0 alone inside
        d = [Draw(mesh=0, material=4, cull=1, world=tuple(ORTHO_WORLD.ravel().tolist()))]
    elif name == "behind":  # (e) every vertex outside, next to one that is drawn
        m, d = [soup([(0.5, 0.2, -3.0), (-0.7, 0.1, -5.0), (0.1, -0.6, -2.5),
                      (-0.8, 0.6, 1.0), (0.9, 0.5, 1.0), (0.0, -0.7, 0.5)], 23)], [Draw(mesh=0, material=5, cull=1)]
    elif name == "nan_vertex":  # (f) a NaN position is outside and poisons its crossings: the pieces are skipped near
        mesh = soup([(-0.8, 0.6, 1.0), (0.9, 0.5, 1.0), (0.0, -0.7, 0.5),
                     (-0.6, 0.4, 0.5), (0.7, 0.3, 0.5), (0.1, -0.5, 0.2),
                     (-0.5, 0.5, 0.8), (0.6, 0.4, -4.0), (0.2, -0.4, 0.3)], 24)
        mesh.vertices[4, 1] = np.nan
        m, d = [mesh], [Draw(mesh=0, material=6, cull=1)]
    elif name == "tiny_and_floor":  # (g) pieces with boxes of a few pixels (the setup lane's path) next to large ones
        e = 0.015
        m = [soup([(0.0, 0.0, -1.85), (e, 0.0, -1.95), (0.0, e, -1.95),
                   (0.05, 0.02, -1.95), (0.05 + e, 0.02, -1.85), (0.05, 0.02 + e, -1.85)], 25), floor(2, 3)]
        d = [Draw(mesh=0, material=7, cull=1), Draw(mesh=1, material=1)]
    elif name == "floor_sphere_floor":  # (h) a clipped floor, a sphere through it, the same floor again (equal z)
        m = [floor(3, 4), S.uv_sphere(12, 6)]
        d = [Draw(mesh=0, material=0), Draw(mesh=1, material=1, world=S.translation(0.3, -0.7, 1.0)),
             Draw(mesh=0, material=2)]
    elif name == "inside_sphere":  # (i) the camera inside a sphere, next to its wall, back faces drawn
        view = camera(W, H, eye=(2.4, 0.5, 0.0), target=(2.4, 0.4, 3.0))
        s = np.diag([3.0, 3.0, 3.0, 1.0]).astype(np.float32)
        m, d = [S.uv_sphere(12, 6)], [Draw(mesh=0, material=8, cull=1, world=tuple(s.ravel().tolist()))]
    elif name == "overview":  # (j) the 58 spheres from the overview camera: nothing crosses the plane
        cfg = S.REFERENCE_SCENE.with_size(W, H).with_camera(*S.OVERVIEW_CAMERA)
        m, d = S.reference_scene_draws(12, 6)
        view = S.reference_scene_view(cfg)
    else:
        raise KeyError(name)
    return m, d, view


CASES = ("floor_quad", "floor_grid") + SINGLE_CASES + ("zero_z", "behind", "nan_vertex", "tiny_and_floor",
                                                       "floor_sphere_floor", "inside_sphere", "overview")


def device_rasterize(ctx, meshes, draws, view, stride=None, rows=None, stream=None, set_meshes=True, flags="clip"):
    """raster_cases.device_rasterize with PBR_RASTER_CLIP_NEAR (`flags` "clip"), through pbr_rasterize_flags with
    another flags word (an int), or through pbr_rasterize (None); returns (planes, material, depth, stats, clip stats),
    synchronised."""
    import torch

    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd.renderer import Attributes

    flags = N.PBR_RASTER_CLIP_NEAR if flags == "clip" else flags
    dev = torch.device("cuda", 0)
    W, H = view.width, view.height
    stride = W + 1 if stride is None else stride
    planes = torch.full((14, H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
    ids = torch.full((H, stride), C.SENTINEL_ID, dtype=torch.int16, device=dev)
    depth = torch.full((H, stride), float(C.SENTINEL), dtype=torch.float32, device=dev)
    if set_meshes:
        ctx.set_meshes(meshes, stream=stream)
    torch.cuda.synchronize()
    if rows is None:
        ctx.rasterize_flags(draws, view, flags, out=(Attributes(planes, ids, width=W), depth), stream=stream)
    else:
        r0, r1 = rows
        ctx.rasterize_flags(draws, view.rows(r0, r1), flags,
                            out=(Attributes(planes[:, r0:r1], ids[r0:r1], width=W), depth[r0:r1]), stream=stream)
    stats, clip = ctx.raster_stats(stream=stream), ctx.raster_clip_stats(stream=stream)
    torch.cuda.synchronize()
    return planes.cpu().numpy(), ids.cpu().numpy().view(np.uint16), depth.cpu().numpy(), stats, clip


BOUNDS_CASES = (("floor_quad", "70x37"), ("tiny_and_floor", "256x64"), ("inside_sphere", "70x37"))


def main(out_path):
    """BOUNDS_CASES, clipped, under the loaded library; the bounds flags of a bounds-checked build."""
    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd.renderer import ShadingContext

    result = {}
    with ShadingContext(0) as ctx:
        for name, frame in BOUNDS_CASES:
            W, H = FRAMES[frame]
            m, d, v = case(name, W, H)
            planes, ids, depth, stats, clip = device_rasterize(ctx, m, d, v)
            key = f"{name}_{frame}"
            result[key + "__planes"], result[key + "__ids"], result[key + "__depth"] = planes, ids, depth
            result[key + "__stats"] = np.array([stats[k] for k in sorted(stats)] + [clip[k] for k in sorted(clip)],
                                               np.int64)
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds", "raster", "mesh")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")  # the raster kernels' unit
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("clipped rasterize under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
