"""One layer of the transparent pass (pbr_rasterize_layer, csrc/raster.h) restated in numpy on
the fragment enumeration of tests/raster_alpha_reference.py (its rasterize() loop with no tested draw: steps 1-6 and 2a
through tests/raster_reference.py and tests/raster_clip_reference.py), flags 0 and PBR_RASTER_CLIP_NEAR: int64 edge
functions, float32 everywhere else, one numpy operation per specified operation. A helper, not a test:
tests/test_raster_layer_host.py checks the restatement against the sequential emulation below and against the rules,
tests/test_gpu_raster_layer.py holds the device to it bit for bit.

    rasterize_layer(meshes, draws, view, depth_in, prim_in=None, clip_near=False)
        -> Layer(planes (14, rows, W) float32, material (rows, W) uint16, depth (rows, W) float32,
                 prim (rows, W) uint32, stats dict, clip stats dict, layer stats dict)
    peel(meshes, draws, view, depth0, clip_near=False) -> [Layer, ...]: layers until one is empty (that one included)
    emulate(meshes, draws, view, depth0, clip_near=False) -> (prims, zs, depth): the D3D pass itself

``emulate`` is the independent statement of what the layers must add up to: the triangles in submission order over a
depth buffer, a fragment accepted iff z < d (LESS, writes on; PBRApp.cpp:830-843 leaves the depth state D3D12_DEFAULT).
``prims[k]`` / ``zs[k]`` hold, per pixel, the k-th accepted fragment's ordinal (-1: none) and z; ``depth`` is the
buffer afterwards. It shares only the fragment enumeration with the restatement: no key, no floor, no atomicMin."""
from collections import namedtuple

import numpy as np

import raster_clip_reference as CR
import raster_reference as R

F = R.F
LAYER_STAT_NAMES = ("layer_fragments",)
NO_FLOOR = np.uint32(0xFFFFFFFF)  # prim_out of a pixel without a winner: no ordinal reaches it
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

Layer = namedtuple("Layer", "planes material depth prim stats clip layer")


def band(view):
    r0 = int(view.row_begin)
    r1 = int(view.height) if view.row_end is None else int(view.row_end)
    return r0, r1


def fragments(meshes, draws, view, clip_near, stats, clip, setups):
    """Steps 1-6 (2a with ``clip_near``) of every triangle of the call, in submission order: yields
    (ordinal, (y0, y1, x0, x1) of its clipped box, fragment mask, z) per triangle or piece that reaches coverage, and
    fills the counters and ``setups`` (ordinal -> [(piece in setup order, A, material)])."""
    W, H = int(view.width), int(view.height)
    r0, r1 = band(view)
    prim = 0
    for dr in draws:
        mesh = meshes[dr.mesh]
        vs = R.vertex_stage(mesh.vertices, dr, view)
        ph = CR.clip_space(mesh.vertices, dr, view)
        count = mesh.indices.size - dr.first_index if dr.index_count is None else dr.index_count
        tri_idx = mesh.indices[dr.first_index:dr.first_index + count].reshape(-1, 3).astype(np.int64)
        for tri in tri_idx:
            t = prim
            prim += 1
            stats["triangles"] += 1
            i = [int(tri[0]), int(tri[1]), int(tri[2])]
            if clip_near:
                n, pieces = CR.pieces_of(vs, ph, view, i)
                if n == 0:
                    stats["skipped_near"] += 1
                    continue
                if n < 3:
                    clip["clipped_near"] += 1
                    clip["clip_pieces"] += len(pieces)
            else:
                pieces = [[CR._PieceVertex(vs, ph, view, k) for k in i]]
            for p in pieces:
                if any(v.near for v in p):
                    stats["skipped_near"] += 1
                    continue
                if any(v.guard for v in p):
                    stats["skipped_guard_band"] += 1
                    continue
                X, Y = [v.X for v in p], [v.Y for v in p]
                A = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
                if A == 0:
                    stats["zero_area"] += 1
                    continue
                if A < 0:
                    if dr.cull == 0:
                        stats["backface_culled"] += 1
                        continue
                    p = [p[0], p[2], p[1]]
                    X, Y = [v.X for v in p], [v.Y for v in p]
                    A = -A
                setups.setdefault(t, []).append((p, A, dr.material))
                x0, x1 = max((min(X) - 128 + 255) >> 8, 0), min((max(X) - 128) >> 8, W - 1)
                y0, y1 = max((min(Y) - 128 + 255) >> 8, r0), min((max(Y) - 128) >> 8, r1 - 1)
                if x0 > x1 or y0 > y1:
                    continue
                y, x = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64),
                                   indexing="ij")
                cov, _, z = CR._coverage(p, A, x, y)
                frag = cov & (z >= F(0)) & (z < F(1))  # NaN: no fragment
                stats["fragments"] += int(frag.sum())
                yield t, (y0 - r0, y1 + 1 - r0, x0, x1 + 1), frag, z


def rasterize_layer(meshes, draws, view, depth_in, prim_in=None, clip_near=False):
    """The whole call. ``depth_in`` (rows, W) float32; ``prim_in`` (rows, W) uint32 or None (floor 0)."""
    W, H = int(view.width), int(view.height)
    r0, r1 = band(view)
    rows = r1 - r0
    depth_in = np.asarray(depth_in, F)
    floor = np.zeros((rows, W), np.uint32) if prim_in is None else np.asarray(prim_in, np.uint32)
    assert depth_in.shape == floor.shape == (rows, W)
    vis = np.full((rows, W), EMPTY, np.uint64)
    stats = dict.fromkeys(R.STAT_NAMES, 0)
    clip = dict.fromkeys(CR.CLIP_STAT_NAMES, 0)
    layer = dict.fromkeys(LAYER_STAT_NAMES, 0)
    setups = {}
    with np.errstate(all="ignore"):
        for t, (ya, yb, xa, xb), frag, z in fragments(meshes, draws, view, clip_near, stats, clip, setups):
            # step 7a: eligible iff prim >= floor and z < depth_in (NaN: never); the key's halves exchanged
            ok = frag & (np.uint32(t) >= floor[ya:yb, xa:xb]) & (z < depth_in[ya:yb, xa:xb])
            layer["layer_fragments"] += int(ok.sum())
            key = (np.uint64(t) << np.uint64(32)) | z.view(np.uint32).astype(np.uint64)
            sub = vis[ya:yb, xa:xb]
            sub[ok] = np.minimum(sub[ok], key[ok])

        planes = np.zeros((14, rows, W), F)
        material = np.full((rows, W), R.NONE, np.uint16)
        yy, xx = np.meshgrid(np.arange(r0, r1, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
        sx = (2 * xx + 1).astype(F) / F(W) - F(1.0)
        sy = F(1.0) - (2 * yy + 1).astype(F) / F(H)
        Fw, Rt, Up, eye = (np.asarray(v, F) for v in (view.bg_forward, view.bg_right, view.bg_up, view.eye))
        d = [(Fw[c] + sx * Rt[c]) + sy * Up[c] for c in range(3)]
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        for c in range(3):
            n = d[c] / length
            planes[3 + c] = n
            planes[c] = eye[c] + n * F(100.0)
        won = vis != EMPTY
        prims = (vis >> np.uint64(32)).astype(np.int64)
        zbits = (vis & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        depth = depth_in.copy()  # a pixel without a winner: depth_in passed through, bits and all
        prim_out = np.full((rows, W), NO_FLOOR, np.uint32)
        prim_out[won] = (prims[won] + 1).astype(np.uint32)
        resolved = np.zeros((rows, W), bool)
        for t in np.unique(prims[won]).tolist():
            todo = won & (prims == t)
            for p, A, mat in setups[t]:  # step 8 / 2a.8: the lowest-numbered piece that covers with the key's z bits
                x, y = xx[todo], yy[todo]
                cov, l, z = CR._coverage(p, A, x, y)
                hit = cov & (z >= F(0)) & (z < F(1)) & (z.view(np.uint32) == zbits[todo])
                m = np.zeros((rows, W), bool)
                m[todo] = hit
                depth[m] = z[hit]
                pr = [l[k][hit] * p[k].rw for k in range(3)]
                s = (pr[0] + pr[1]) + pr[2]
                q = [pr[k] / s for k in range(3)]
                for k in range(14):
                    planes[k][m] = (q[0] * p[0].attribute(k) + q[1] * p[1].attribute(k)) + q[2] * p[2].attribute(k)
                material[m] = mat
                resolved |= m
                todo = todo & ~m
    assert np.array_equal(resolved, won)
    assert np.array_equal(depth[won].view(np.uint32), zbits[won])
    return Layer(planes, material, depth, prim_out, stats, clip, layer)


def peel(meshes, draws, view, depth0, clip_near=False, max_layers=64):
    """Layers from ``depth0`` on, each fed the previous one's depth and floor, until one issues no update; that empty
    layer is the last element."""
    layers = []
    depth, prim = np.asarray(depth0, F), None
    for _ in range(max_layers):
        layers.append(rasterize_layer(meshes, draws, view, depth, prim, clip_near))
        if layers[-1].layer["layer_fragments"] == 0:
            return layers
        depth, prim = layers[-1].depth, layers[-1].prim
    raise AssertionError("no empty layer within max_layers")


def emulate(meshes, draws, view, depth0, clip_near=False):
    """The transparent pass as the output merger runs it: fragments in submission order, accepted iff z < d, d = z."""
    depth = np.array(depth0, F)
    count = np.zeros(depth.shape, np.int64)
    prims, zs = [], []
    stats, clip = dict.fromkeys(R.STAT_NAMES, 0), dict.fromkeys(CR.CLIP_STAT_NAMES, 0)
    with np.errstate(all="ignore"):
        for t, (ya, yb, xa, xb), frag, z in fragments(meshes, draws, view, clip_near, stats, clip, {}):
            d = depth[ya:yb, xa:xb]
            accept = frag & (z < d)
            if not accept.any():
                continue
            c = count[ya:yb, xa:xb]
            for level in np.unique(c[accept]).tolist():
                while len(prims) <= level:
                    prims.append(np.full(depth.shape, -1, np.int64))
                    zs.append(np.full(depth.shape, np.nan, F))
                m = accept & (c == level)
                prims[level][ya:yb, xa:xb][m] = t
                zs[level][ya:yb, xa:xb][m] = z[m]
            d[accept] = z[accept]
            c[accept] += 1
    return prims, zs, depth
