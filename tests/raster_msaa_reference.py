"""Four samples per pixel (pbr_msaa_rasterize, pbr_msaa_fragments, pbr_msaa_resolve) restated
in numpy on top of tests/raster_reference.py's helpers: one numpy operation per specified operation, int64 edge
functions, float32 everywhere else. A helper, not a test: tests/test_raster_msaa_host.py checks the restatement against
the rules and against the 1x restatement, tests/test_gpu_raster_msaa.py and tests/test_gpu_msaa_resolve.py hold the
device to it bit for bit.

    sample_keys(meshes, draws, view)      -> Samples(vis (4, rows, W) uint64, stats, setups)
    slots_of(vis)                         -> (slot (4, rows, W) int, n (rows, W) int, owner (rows, W) uint8)
    fragments(samples, view, slot)        -> (planes (14, rows, W), material, depth, owner, slot_pixels)
    resolve(frames, owner, n_slots, fmt)  -> the resolved frame, float32 or uint8"""
from collections import namedtuple

import numpy as np

import raster_reference as R

F = np.float32
OFFSETS = ((-2, -6), (6, -2), (-6, 2), (2, 6))  # (dx, dy) of sample s in 1/16 pixel: D3D's standard 4x pattern
RGBA32F, RGBA8 = 0, 1

Samples = namedtuple("Samples", "vis stats setups")


def edge_values_at(edges, px, py):
    """The three edge functions at the points (px, py) of the 1/256 grid (int64 arrays)."""
    return [np.int64(dx) * (py - np.int64(ya)) - np.int64(dy) * (px - np.int64(xa)) for dx, dy, xa, ya, _ in edges]


def sample_keys(meshes, draws, view, coverage_counts=None):
    """Steps 1-4 as raster_reference.rasterize, then steps 5-7 at the four sample points. ``coverage_counts``: an
    optional (4, rows, W) int array that receives, per sample, how many triangles' coverage tests it passed."""
    W, H = int(view.width), int(view.height)
    r0 = int(view.row_begin)
    r1 = H if view.row_end is None else int(view.row_end)
    rows = r1 - r0
    vis = np.full((4, rows, W), R.EMPTY, np.uint64)
    stats = dict.fromkeys(R.STAT_NAMES, 0)
    setups = {}
    prim = 0
    with np.errstate(all="ignore"):
        for dr in draws:
            mesh = meshes[dr.mesh]
            vs = R.vertex_stage(mesh.vertices, dr, view)
            count = mesh.indices.size - dr.first_index if dr.index_count is None else dr.index_count
            tri_idx = mesh.indices[dr.first_index:dr.first_index + count].reshape(-1, 3).astype(np.int64)
            for tri in tri_idx:
                t = prim
                prim += 1
                stats["triangles"] += 1
                i = [int(tri[0]), int(tri[1]), int(tri[2])]
                if vs["near"][i].any():
                    stats["skipped_near"] += 1
                    continue
                if vs["guard"][i].any():
                    stats["skipped_guard_band"] += 1
                    continue
                X = [int(vs["X"][k]) for k in i]
                Y = [int(vs["Y"][k]) for k in i]
                A = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
                if A == 0:
                    stats["zero_area"] += 1
                    continue
                if A < 0:
                    if dr.cull == 0:
                        stats["backface_culled"] += 1
                        continue
                    i[1], i[2] = i[2], i[1]
                    X[1], X[2] = X[2], X[1]
                    Y[1], Y[2] = Y[2], Y[1]
                    A = -A
                setups[t] = (vs, i, A, dr.material)
                # every pixel the bounding box touches and one more on each side: generous, not the device's box
                x0, x1 = max((min(X) >> 8) - 1, 0), min((max(X) >> 8) + 1, W - 1)
                y0, y1 = max((min(Y) >> 8) - 1, r0), min((max(Y) >> 8) + 1, r1 - 1)
                if x0 > x1 or y0 > y1:
                    continue
                y, x = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64),
                                   indexing="ij")
                edges = R._edges(X, Y)
                zv = [vs["z"][k] for k in i]
                for s, (dx, dy) in enumerate(OFFSETS):
                    E = edge_values_at(edges, np.int64(256) * x + np.int64(128 + 16 * dx),
                                       np.int64(256) * y + np.int64(128 + 16 * dy))
                    cov = np.ones(x.shape, bool)
                    for e, (_, _, _, _, top_left) in zip(E, edges):
                        cov &= (e > 0) | ((e == 0) & top_left)
                    if coverage_counts is not None:
                        coverage_counts[s, y0 - r0:y1 + 1 - r0, x0:x1 + 1] += cov
                    z = R._z(R._barycentrics(E, A), zv).astype(F)
                    frag = cov & (z >= F(0)) & (z < F(1))  # NaN: no fragment
                    stats["fragments"] += int(frag.sum())
                    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
                    sub = vis[s, y0 - r0:y1 + 1 - r0, x0:x1 + 1]
                    sub[frag] = np.minimum(sub[frag], key[frag])
    return Samples(vis, stats, setups)


def slots_of(vis):
    """Per sample its slot, per pixel the slot count and the owner byte: samples with the same low word (a triangle's
    ordinal, or all ones for none) are one fragment; slots are numbered by their lowest sample."""
    ident = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    slot = np.zeros(vis.shape, np.int64)
    n = np.ones(vis.shape[1:], np.int64)
    for s in range(1, 4):
        found = np.zeros(vis.shape[1:], bool)
        for p in range(s):
            same = ~found & (ident[s] == ident[p])
            slot[s][same] = slot[p][same]
            found |= same
        slot[s][~found] = n[~found]
        n[~found] += 1
    owner = sum(slot[s] << (2 * s) for s in range(4)).astype(np.uint8)
    return slot, n, owner


def background(view):
    """Step 9's planes for the band (raster_reference.rasterize's operations)."""
    W, H = int(view.width), int(view.height)
    r0 = int(view.row_begin)
    r1 = H if view.row_end is None else int(view.row_end)
    planes = np.zeros((14, r1 - r0, W), F)
    yy, xx = np.meshgrid(np.arange(r0, r1, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    with np.errstate(all="ignore"):
        sx = (2 * xx + 1).astype(F) / F(W) - F(1.0)
        sy = F(1.0) - (2 * yy + 1).astype(F) / F(H)
        Fw, Rt, Up, eye = (np.asarray(v, F) for v in (view.bg_forward, view.bg_right, view.bg_up, view.eye))
        d = [(Fw[c] + sx * Rt[c]) + sy * Up[c] for c in range(3)]
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        for c in range(3):
            n = d[c] / length
            planes[3 + c] = n
            planes[c] = eye[c] + n * F(100.0)
    return planes, xx, yy


def fragments(samples, view, slot):
    """Slot ``slot`` of every pixel: (planes, material, depth, owner, slot_pixels). Attributes: step 8 at the pixel
    centre with the triangle of the slot's lowest sample, covered or not; depth: the high word of that sample's key."""
    vis, setups = samples.vis, samples.setups
    sl, n, owner = slots_of(vis)
    planes, xx, yy = background(view)
    material = np.full(vis.shape[1:], R.NONE, np.uint16)
    depth = np.ones(vis.shape[1:], F)
    key = np.full(vis.shape[1:], R.EMPTY, np.uint64)
    for s in (3, 2, 1, 0):  # the lowest sample of the slot is written last
        m = sl[s] == slot
        key[m] = vis[s][m]
    won = (n > slot) & (key != R.EMPTY)
    prims = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
    with np.errstate(all="ignore"):
        for t in np.unique(prims[won]).tolist():
            vs, i, A, mat = setups[t]
            m = won & (prims == t)
            x, y = xx[m], yy[m]
            E = R._edge_values(R._edges([int(vs["X"][k]) for k in i], [int(vs["Y"][k]) for k in i]), x, y)
            l = R._barycentrics(E, A)
            p = [l[k] * vs["rw"][i[k]] for k in range(3)]
            s_ = (p[0] + p[1]) + p[2]
            q = [p[k] / s_ for k in range(3)]
            for k in range(14):
                a = vs["a"][k]
                planes[k][m] = (q[0] * a[i[0]] + q[1] * a[i[1]]) + q[2] * a[i[2]]
            material[m] = mat
    depth[won] = (key[won] >> np.uint64(32)).astype(np.uint32).view(F)
    slot_pixels = [int((n > k).sum()) for k in range(4)]
    return planes, material, depth, owner, slot_pixels


def unorm8(c):
    """pbr_unorm.h: NaN -> 0, clamp to [0, 1], c * 255 + 0.5 in float32, truncate."""
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        c = np.where(c == c, c, F(0))
        c = np.where(c > F(1), F(1), c)
        c = np.where(c < F(0), F(0), c)
        return (c * F(255.0) + F(0.5)).astype(np.uint32).astype(np.uint8)


def saturate(c):
    """pbr_blend_layer's clamp: NaN -> 0, then to [0, 1]."""
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        c = np.where(c == c, c, F(0))
        c = np.where(c > F(1), F(1), c)
        return np.where(c < F(0), F(0), c).astype(F)


def resolve(frames, owner, n_slots, fmt=RGBA32F):
    """((c_0 + c_1) + (c_2 + c_3)) * 0.25f per channel, c_s the pixel of frame (owner >> 2s) & 3, 0 for a slot >=
    n_slots (that frame is not looked at). RGBA8: each c_s through unorm8(clamp()) and / 255.0f first, unorm8 after."""
    owner = np.asarray(owner, np.uint8)
    c = []
    for s in range(4):
        k = (owner >> np.uint8(2 * s)) & np.uint8(3)
        cs = np.zeros(owner.shape + (4,), F)
        for j in range(min(int(n_slots), 4)):
            m = k == j
            if m.any():
                cs[m] = np.asarray(frames[j], F)[m]
        c.append(cs)
    with np.errstate(all="ignore"):
        if fmt == RGBA8:
            c = [unorm8(saturate(cs)).astype(F) / F(255.0) for cs in c]
        out = ((c[0] + c[1]) + (c[2] + c[3])) * F(0.25)
    return unorm8(out) if fmt == RGBA8 else out.astype(F)
