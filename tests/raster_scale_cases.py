"""Inputs of tests/test_gpu_raster_scale.py and tests/test_frontend_shapes_host.py: scenes that take the rasteriser's
list, box and draw-table code ("Kernels") past the sizes the scenes of tests/raster_cases.py reach: a
large list longer than the large kernel's 1,024 striding workgroups, triangle counts around the setup kernel's workgroup
of 256, clipped boxes of exactly 64 and 65 pixels, a box of more than 32 blocks whose origin is off the 64x4 grid, a
draw table of 300 draws with empty ones, and coordinates next to the 2^23-subpixel guard band. A helper, not a test. Run
as a script (bounds_runs() under whatever library PBR_LIB_PATH names -- the bounds-checked build, in a fresh child
process, as tests/raster_cases.py does) it writes the device results and the bounds flags to the .npz given."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_alpha_cases as AC  # noqa: E402
import raster_cases as C  # noqa: E402
import raster_clip_reference as CR  # noqa: E402
import raster_reference as R  # noqa: E402
from physically_based_renderer_amd import scenes as S  # noqa: E402
from physically_based_renderer_amd.renderer import Draw  # noqa: E402

FRAME = (71, 37)
SMALL_PIXELS, LARGE_GRID_X, LARGE_SLABS, BLOCK_W, BLOCK_H = 64, 1024, 32, 64, 4  # csrc/raster.h
N_SLIVERS = 1300


# ---- many_large -------------------------------------------------------------------------------------------------------

def many_large(clip=False, n=N_SLIVERS):
    """(meshes, draws, view) at 71x37: `n` slivers, each from left of the frame to right of it over 2 to 4 rows, the
    third vertex at random, w in [0.5, 2], cull none: every clipped box is wider than 64 pixels, so every triangle is on
    the large list. ``clip``: every tenth sliver's third vertex has w = 0.05, behind the near plane (w = 0.1 under
    raster_cases.PERSP), and sits in the left part of the frame: the sliver is cut into two pieces, both with a box
    above 64 pixels, so second pieces are listed (the piece number in bit 31 of the entry)."""
    W, H = FRAME
    rng = np.random.default_rng(0x51C3)
    q = lambda f: np.floor(f * 256) / 256  # noqa: E731
    y0 = q(rng.uniform(0.0, H - 4.0, n))
    rows = rng.uniform(2.0, 4.0, n)
    xl, xr = q(rng.uniform(-3.0, -0.5, n)), q(rng.uniform(W + 0.5, W + 3.0, n))
    yr = q(y0 + rng.uniform(0.0, 0.5, n))
    x2, y2 = q(rng.uniform(1.0, W - 1.0, n)), q(y0 + rows)
    w = rng.uniform(0.5, 2.0, (n, 3))
    if clip:
        cut = np.arange(n) % 10 == 3
        w[cut, 2] = 0.05
        x2 = np.where(cut, q(rng.uniform(1.0, 30.0, n)), x2)
    pts = np.stack([np.stack([xl, y0, w[:, 0]], -1), np.stack([xr, yr, w[:, 1]], -1), np.stack([x2, y2, w[:, 2]], -1)],
                   1)
    m, d = C.one_draw(pts.reshape(-1, 3), W, H, 61, material=0, cull=1)
    return m, d, C.screen_view(W, H)


def cut_to(draws, n_tris):
    """The single draw of a scene cut to its first `n_tris` triangles."""
    d = draws[0]
    return [Draw(mesh=d.mesh, material=d.material, cull=d.cull, index_count=3 * n_tris)]


def checker_table():
    """(materials, textures): material 0 is tested against a 4x4 checkerboard."""
    return [AC.tested(0), AC.opaque()], [AC.checker(4, 4)]


def tri_counts(n_tris):
    """raster_cases' random_subpixel at 71x37 cut to `n_tris` triangles: 255, 256 and 257 are the last lane of the setup
    kernel's first workgroup, a full workgroup and one lane of a second."""
    m, d, v = C.case("random_subpixel", *FRAME)
    return m, [Draw(mesh=0, material=d[0].material, cull=d[0].cull, index_count=3 * n_tris)], v


# ---- box_threshold ----------------------------------------------------------------------------------------------------

# (x, y, width, height) of each triangle's clipped box in the full 71x37 frame, in triangle order: four of exactly 64
# pixels (the setup lane's loop), three of 65 and one of 66 (33x2, the smallest two-row box above 64; the large list),
# and one 20 columns wide that the frame's right edge cuts to 8x8.
BOXES = ((2, 2, 8, 8), (3, 12, 64, 1), (20, 2, 16, 4), (40, 3, 2, 32),
         (3, 14, 65, 1), (45, 3, 13, 5), (60, 10, 5, 13), (5, 30, 33, 2), (63, 20, 8, 8))
UNCUT_WIDTH = {8: 20}  # triangle 8 spans 20 columns before the frame cuts it
BOX_BANDS = ((0, 6), (6, 20), (20, 31), (31, 37))
# (triangle, band): large in the full frame, small (and not empty) in that band
LARGE_TO_SMALL = ((5, (0, 6)), (6, (6, 20)), (7, (20, 31)))


def box_threshold():
    """Right triangles whose legs put exactly BOXES' pixel centres inside their bounding boxes; w grows with the
    triangle's number, so the earlier one is nearer where two overlap."""
    W, H = FRAME
    pts = []
    for k, (x, y, bw, bh) in enumerate(BOXES):
        bw = UNCUT_WIDTH.get(k, bw)
        w = 1.0 + 0.1 * k
        pts += [(x + 0.25, y + 0.25, w), (x + bw + 0.25, y + 0.25, w), (x + 0.25, y + bh + 0.25, w)]
    m, d = C.one_draw(pts, W, H, 62)
    return m, d, C.screen_view(W, H)


# ---- offset_blocks ----------------------------------------------------------------------------------------------------

OFFSET_FRAME = (150, 75)
OFFSET_BANDS = ((7, 30), (30, 75))


def offset_blocks():
    """One triangle whose box runs from (3, 5) to (140, 70) -- 3 x 17 = 51 blocks of 64x4, more than the 32 slabs, its
    origin off the block grid -- and a smaller, nearer one inside it."""
    W, H = OFFSET_FRAME
    m, d = C.one_draw([(3.25, 5.25, 2.0), (141.25, 5.25, 1.5), (3.25, 71.25, 1.0),
                       (30.25, 20.25, 0.8), (100.25, 25.25, 0.9), (50.25, 60.25, 0.7)], W, H, 63)
    return m, d, C.screen_view(W, H)


# ---- many_draws -------------------------------------------------------------------------------------------------------

N_DRAWS = 300
COUNT_CYCLE = (0, 3, 6, 0, 0, 3)


def many_draws(all_empty=False):
    """300 draws over two small meshes at 71x37: index_count cycles through 0, 3, 6, 0, 0, 3 (the last draw is empty
    too), so the triangle prefix has equal entries first, last and in runs of two; first_index, world, tex_transform,
    material and cull change from draw to draw. ``all_empty``: every index_count is 0."""
    W, H = FRAME
    a = C.soup([(4, 3, 1), (W * 0.5, 6, 1.5), (9, H * 0.6, 1), (W * 0.4, H * 0.3, 2), (W * 0.8, H * 0.4, 1),
                (W * 0.45, H * 0.9, 1.2), (W - 5, 4, 0.8), (W - 9, H - 3, 0.8), (W * 0.6, H * 0.5, 0.9),
                (12, H - 4, 1.1), (W * 0.3, 5, 1.3), (W * 0.7, H - 2, 0.6)], W, H, 64)
    cx, cy = W // 2 + 0.5, H // 2 + 0.5
    b = C.soup(C.fan_points(cx, cy, C.fan_rim(cx, cy, W, H), 1.4), W, H, 65)
    draws = []
    for k in range(N_DRAWS):
        count = 0 if all_empty or k == N_DRAWS - 1 else COUNT_CYCLE[k % len(COUNT_CYCLE)]
        mesh = k % 2
        n_idx = (a, b)[mesh].indices.size
        first = 3 * ((k * 5) % ((n_idx - 6) // 3 + 1))
        world = S.translation(0.03 * (k % 7) - 0.09, 0.05 * (k % 5) - 0.1, 0.0)
        tex = AC.scale_translate(1.0 + (k % 3), 2.0 - 0.5 * (k % 4), 0.125 * (k % 8), -0.25 * (k % 3))
        draws.append(Draw(mesh=mesh, material=k % 11, cull=(k // 3) % 2, first_index=first, index_count=count,
                          world=world, tex_transform=tex))
    return [a, b], draws, C.screen_view(W, H)


def tri_prefix(draws):
    """The triangle prefix the host builds: entry d is the number of triangles before draw d."""
    return np.concatenate([[0], np.cumsum([dr.index_count // 3 for dr in draws])]).astype(np.int64)


# ---- guard_scale ------------------------------------------------------------------------------------------------------

BEYOND = 3  # the triangle of guard_scale with a vertex beyond the band


def guard_scale(clip=False):
    """Three triangles at 71x37 with vertices 20,000 to 32,700 pixels out that cover part of the frame, one of them with
    a vertex at 32,767.9 pixels (inside the 2^23-subpixel band: drawn), and raster_cases' triangle with a vertex at
    40,000 pixels (beyond it: skipped). ``clip``: the first triangle's third vertex is behind the near plane."""
    W, H = FRAME
    pts = [(-25000, -20010, 1.0), (30000, 24020, 1.5), (-20000, 30000, 0.05 if clip else 0.8),  # below a diagonal
           (-32700, 10, 1.2), (20, -31000, 0.9), (32767.9, 25, 1.8),                             # above y ~ 17.5
           (50, -20500, 0.7), (32000, 100, 0.6), (20, 32700, 1.1),                               # right of x ~ 35
           (5, 5, 1), (40000, 8, 1), (12, 30, 1)]
    m, d = C.one_draw(pts, W, H, 66, cull=1)
    return m, d, C.screen_view(W, H)


# ---- what a scene lists -----------------------------------------------------------------------------------------------

def boxes(meshes, draws, view, clip=False):
    """[(prim, piece, x0, y0, width, height)] of every triangle (with ``clip``: piece) that passes setup with a
    non-empty clipped box (DESIGN.md §12 step 4 and the box of "Kernels": the pixel centres inside the bounding box,
    clipped to the frame's width and the view's row band), in submission order."""
    W, H = int(view.width), int(view.height)
    r0, r1 = int(view.row_begin), H if view.row_end is None else int(view.row_end)
    out, prim = [], 0
    for dr in draws:
        mesh = meshes[dr.mesh]
        vs = R.vertex_stage(mesh.vertices, dr, view)
        ph = CR.clip_space(mesh.vertices, dr, view) if clip else None
        count = mesh.indices.size - dr.first_index if dr.index_count is None else dr.index_count
        for tri in mesh.indices[dr.first_index:dr.first_index + count].reshape(-1, 3).astype(np.int64):
            i = [int(t) for t in tri]
            if clip:
                pieces = [([v.X for v in p], [v.Y for v in p], any(v.near or v.guard for v in p))
                          for p in CR.pieces_of(vs, ph, view, i)[1]]
            else:
                pieces = [([int(vs["X"][k]) for k in i], [int(vs["Y"][k]) for k in i],
                           bool(vs["near"][i].any() or vs["guard"][i].any()))]
            for piece, (X, Y, skipped) in enumerate(pieces):
                A = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
                if skipped or A == 0 or (A < 0 and dr.cull == 0):
                    continue
                x0, x1 = max((min(X) - 128 + 255) >> 8, 0), min((max(X) - 128) >> 8, W - 1)
                y0, y1 = max((min(Y) - 128 + 255) >> 8, r0), min((max(Y) - 128) >> 8, r1 - 1)
                if x0 <= x1 and y0 <= y1:
                    out.append((prim, piece, x0, y0, x1 - x0 + 1, y1 - y0 + 1))
            prim += 1
    return out


def listed(bs):
    """The entries of boxes() that go to the large list: more than 64 pixels."""
    return [b for b in bs if b[4] * b[5] > SMALL_PIXELS]


def blocks(b):
    """(nbx, nby) of a box: its 64x4 blocks, counted from the box's own origin."""
    return (b[4] - 1) // BLOCK_W + 1, (b[5] - 1) // BLOCK_H + 1


# ---- the bounds-checked build -----------------------------------------------------------------------------------------

def bounds_runs():
    """[(name, meshes, draws, view, materials, textures, clip_near, alpha_test)] the bounds-checked build runs."""
    mats, texs = checker_table()
    return [("many_large_plain",) + many_large() + ([], [], False, False),
            ("many_large_clip_alpha",) + many_large(clip=True) + (mats, texs, True, True),
            ("many_draws",) + many_draws() + ([], [], False, False)]


def main(out_path):
    """bounds_runs() under the loaded library; the bounds flags of a bounds-checked build."""
    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd.renderer import ShadingContext

    result = {}
    with ShadingContext(0) as ctx:
        for name, m, d, v, mats, texs, clip_near, alpha_test in bounds_runs():
            planes, ids, depth, stats, clip, alpha = AC.device_rasterize(ctx, m, d, v, mats, texs, clip_near, alpha_test)
            result[name + "__planes"], result[name + "__ids"], result[name + "__depth"] = planes, ids, depth
            result[name + "__stats"] = np.array([stats[k] for k in sorted(stats)] + [clip[k] for k in sorted(clip)] +
                                                [alpha[k] for k in sorted(alpha)], np.int64)
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds", "raster", "mesh")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")  # the raster kernels' unit
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("scale cases under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
