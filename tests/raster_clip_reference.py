"""Near-plane clipping of the rasteriser (pbr_rasterize_flags with PBR_RASTER_CLIP_NEAR,
csrc/raster.h) restated in numpy on top of tests/raster_reference.py: one numpy operation per specified operation.
A helper, not a test: tests/test_raster_clip_host.py checks the restatement against the rules it encodes,
tests/test_gpu_raster_clip.py holds the device to it bit for bit.

    rasterize(meshes, draws, view) -> (planes (14, rows, W) float32, material (rows, W) uint16,
                                       depth (rows, W) float32, stats dict, clip stats dict)

always with the flag set; the unflagged call is raster_reference.rasterize."""
import numpy as np

import raster_reference as R

F = R.F
CLIP_STAT_NAMES = ("clipped_near", "clip_pieces")


def clip_space(vertices, draw, view):
    """PosH of step 1 for every vertex of a mesh under one draw, (4, n): the operations of R.vertex_stage again."""
    v = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 14)
    one = np.ones(v.shape[0], F)
    with np.errstate(all="ignore"):
        pw = R.mul4(v[:, 0], v[:, 1], v[:, 2], one, R._m(draw.world))
        return np.array(R.mul4(pw[0], pw[1], pw[2], pw[3], R._m(view.view_proj)), F)


def viewport(x, y, z, w, view):
    """Steps 2-3 on one clip-space position (float32 scalars): (X, Y, ndc z, rw, near, guard)."""
    with np.errstate(all="ignore"):
        near = not (w > F(0))
        ndx, ndy, ndz = x / w, y / w, z / w
        xs = (ndx * F(0.5) + F(0.5)) * F(view.width)
        ys = (F(0.5) - ndy * F(0.5)) * F(view.height)
        tx, ty = xs * F(256.0), ys * F(256.0)
        inside = bool(np.abs(tx) < F(2.0 ** 23)) and bool(np.abs(ty) < F(2.0 ** 23))  # False for NaN and inf
        X = int(np.rint(tx)) if inside else 0
        Y = int(np.rint(ty)) if inside else 0
        rw = F(1.0) / w
    return X, Y, F(ndz), F(rw), near, not inside


class _PieceVertex:
    """A vertex of a piece: a submitted vertex `a` (b None), or the crossing of the edge from the inside vertex `a`
    to the outside vertex `b`, always computed in that direction."""

    def __init__(self, vs, ph, view, a, b=None):
        self.a, self.b, self.vs = a, b, vs
        if b is None:
            self.X, self.Y, self.z, self.rw = int(vs["X"][a]), int(vs["Y"][a]), vs["z"][a], vs["rw"][a]
            self.near, self.guard, self.t = bool(vs["near"][a]), bool(vs["guard"][a]), None
            return
        with np.errstate(all="ignore"):
            pa, pb = ph[:, a], ph[:, b]
            self.t = t = pa[2] / (pa[2] - pb[2])
            x = pa[0] + t * (pb[0] - pa[0])
            y = pa[1] + t * (pb[1] - pa[1])
            w = pa[3] + t * (pb[3] - pa[3])
        self.X, self.Y, self.z, self.rw, self.near, self.guard = viewport(x, y, F(0.0), w, view)

    def attribute(self, k):
        a = self.vs["a"][k]
        if self.b is None:
            return a[self.a]
        with np.errstate(all="ignore"):
            return a[self.a] + self.t * (a[self.b] - a[self.a])


def pieces_of(vs, ph, view, i):
    """Rule 2a on the source triangle with vertex indices i: (number of inside vertices, its pieces in order)."""
    V = lambda a, b=None: _PieceVertex(vs, ph, view, a, b)  # noqa: E731
    inside = [bool(ph[2, k] >= F(0.0)) for k in i]  # NaN: outside; -0.0f: inside
    n = sum(inside)
    if n == 3:
        return n, [[V(i[0]), V(i[1]), V(i[2])]]
    if n == 0:
        return n, []
    if n == 1:
        s = inside.index(True)
        vi, vj, vk = i[s], i[(s + 1) % 3], i[(s + 2) % 3]
        return n, [[V(vi), V(vi, vj), V(vi, vk)]]
    s = inside.index(False)
    vi, vj, vk = i[s], i[(s + 1) % 3], i[(s + 2) % 3]
    return n, [[V(vj, vi), V(vj), V(vk)], [V(vj, vi), V(vk), V(vk, vi)]]


def _coverage(p, A, x, y):
    """(covered, z) of a set-up piece at the centres of pixels (x, y)."""
    X, Y = [v.X for v in p], [v.Y for v in p]
    edges = R._edges(X, Y)
    E = R._edge_values(edges, x, y)
    cov = np.ones(x.shape, bool)
    for e, (_, _, _, _, top_left) in zip(E, edges):
        cov &= (e > 0) | ((e == 0) & top_left)
    l = R._barycentrics(E, A)
    z = R._z(l, [v.z for v in p]).astype(F)
    return cov, l, z


def rasterize(meshes, draws, view, coverage_counts=None, details=None):
    """The whole flagged call. ``coverage_counts``: an optional (rows, W) int array that receives, per pixel, how many
    pieces' coverage tests it passed (before the depth range). ``details``: an optional dict that receives ``drawn``,
    the number of triangles and pieces that reached coverage (the counter identity's missing term), and
    ``new_vertices``, the _PieceVertex of every crossing built."""
    W, H = int(view.width), int(view.height)
    r0 = int(view.row_begin)
    r1 = H if view.row_end is None else int(view.row_end)
    rows = r1 - r0
    vis = np.full((rows, W), R.EMPTY, np.uint64)
    stats = dict.fromkeys(R.STAT_NAMES, 0)
    clip = dict.fromkeys(CLIP_STAT_NAMES, 0)
    setups = {}  # prim -> [(piece in setup order, A, material)] in piece order
    new_vertices = []
    prim = 0
    with np.errstate(all="ignore"):
        for dr in draws:
            mesh = meshes[dr.mesh]
            vs = R.vertex_stage(mesh.vertices, dr, view)
            ph = clip_space(mesh.vertices, dr, view)
            count = mesh.indices.size - dr.first_index if dr.index_count is None else dr.index_count
            tri_idx = mesh.indices[dr.first_index:dr.first_index + count].reshape(-1, 3).astype(np.int64)
            for tri in tri_idx:
                t = prim
                prim += 1
                stats["triangles"] += 1
                n, pieces = pieces_of(vs, ph, view, [int(tri[0]), int(tri[1]), int(tri[2])])
                if n == 0:
                    stats["skipped_near"] += 1
                    continue
                if n < 3:
                    clip["clipped_near"] += 1
                    clip["clip_pieces"] += len(pieces)
                for p in pieces:
                    new_vertices += [v for v in p if v.b is not None]
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
                    cov, _, z = _coverage(p, A, x, y)
                    if coverage_counts is not None:
                        coverage_counts[y0 - r0:y1 + 1 - r0, x0:x1 + 1] += cov
                    frag = cov & (z >= F(0)) & (z < F(1))  # NaN: no fragment
                    stats["fragments"] += int(frag.sum())
                    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
                    sub = vis[y0 - r0:y1 + 1 - r0, x0:x1 + 1]
                    sub[frag] = np.minimum(sub[frag], key[frag])

        planes = np.zeros((14, rows, W), F)
        material = np.full((rows, W), R.NONE, np.uint16)
        depth = np.ones((rows, W), F)
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
        won = vis != R.EMPTY
        prims = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
        zbits = (vis >> np.uint64(32)).astype(np.uint32)
        resolved = np.zeros((rows, W), bool)
        for t in np.unique(prims[won]).tolist():
            todo = won & (prims == t)
            for p, A, mat in setups[t]:  # step 8 of 2a: the lowest-numbered piece that made the key
                x, y = xx[todo], yy[todo]
                cov, l, z = _coverage(p, A, x, y)
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
    if details is not None:
        details["drawn"] = sum(len(v) for v in setups.values())
        details["new_vertices"] = new_vertices
    assert np.array_equal(resolved, won)
    assert np.array_equal(depth[won].view(np.uint32), zbits[won])
    return planes, material, depth, stats, clip
