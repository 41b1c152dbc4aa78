"""The rasteriser's semantics (pbr_rasterize, csrc/raster.h) restated in numpy: one numpy operation
per specified operation, int64 edge functions, float32 everywhere else. A helper, not a test: tests/test_raster_host.py
checks the restatement against the rules it encodes, tests/test_gpu_raster.py holds the device to it bit for bit.

    rasterize(meshes, draws, view) -> (planes (14, rows, W) float32, material (rows, W) uint16,
                                       depth (rows, W) float32, stats dict)

with ``meshes`` / ``draws`` / ``view`` the renderer's Mesh / Draw / View."""
import numpy as np

F = np.float32
NONE = 0xFFFF
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
STAT_NAMES = ("triangles", "backface_culled", "zero_area", "skipped_near", "skipped_guard_band", "fragments")


def _m(m):
    return np.asarray(m, dtype=F).reshape(4, 4)


def mul4(x, y, z, w, M):
    """mul(float4, M) for row vectors: the 4-wide dot ((x + y) + z) + w per column."""
    return [((x * M[0, j] + y * M[1, j]) + z * M[2, j]) + w * M[3, j] for j in range(4)]


def mul3(x, y, z, M):
    """mul(float3, (float3x3)M)."""
    return [(x * M[0, j] + y * M[1, j]) + z * M[2, j] for j in range(3)]


def vertex_stage(vertices, draw, view):
    """Steps 1-3 for every vertex of a mesh under one draw: (X, Y int64, z, rw, a (14, n), near, guard)."""
    v = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 14)
    n = v.shape[0]
    Wm, Tm, Mm, VP = _m(draw.world), _m(draw.tex_transform), _m(draw.mat_transform), _m(view.view_proj)
    one, zero = np.ones(n, F), np.zeros(n, F)
    with np.errstate(all="ignore"):
        pw = mul4(v[:, 0], v[:, 1], v[:, 2], one, Wm)
        a = np.empty((14, n), F)
        a[0:3] = pw[0:3]
        a[3:6] = mul3(v[:, 3], v[:, 4], v[:, 5], Wm)
        a[6:9] = mul3(v[:, 6], v[:, 7], v[:, 8], Wm)
        a[9:12] = mul3(v[:, 9], v[:, 10], v[:, 11], Wm)
        ph = mul4(pw[0], pw[1], pw[2], pw[3], VP)
        tc = mul4(v[:, 12], v[:, 13], zero, one, Tm)
        a[12:14] = mul4(tc[0], tc[1], tc[2], tc[3], Mm)[0:2]
        w = ph[3]
        near = ~(w > F(0))
        ndx, ndy, ndz = ph[0] / w, ph[1] / w, ph[2] / w
        xs = (ndx * F(0.5) + F(0.5)) * F(view.width)
        ys = (F(0.5) - ndy * F(0.5)) * F(view.height)
        tx, ty = xs * F(256.0), ys * F(256.0)
        inside = (np.abs(tx) < F(2.0 ** 23)) & (np.abs(ty) < F(2.0 ** 23))  # False for NaN and inf
        X = np.where(inside, np.rint(np.where(inside, tx, F(0))), F(0)).astype(np.int64)
        Y = np.where(inside, np.rint(np.where(inside, ty, F(0))), F(0)).astype(np.int64)
        rw = F(1.0) / w
    return dict(X=X, Y=Y, z=ndz.astype(F), rw=rw.astype(F), a=a, near=near, guard=~inside)


def _edges(X, Y):
    """Per edge k (E0 = 1->2, E1 = 2->0, E2 = 0->1): (dx, dy, xa, ya, top_left), Python ints."""
    out = []
    for k in range(3):
        va, vb = (k + 1) % 3, (k + 2) % 3
        dx, dy = X[vb] - X[va], Y[vb] - Y[va]
        out.append((dx, dy, X[va], Y[va], dy < 0 or (dy == 0 and dx > 0)))
    return out


def _edge_values(edges, x, y):
    """The three edge functions at the centres of pixels (x, y) (int64 arrays)."""
    px, py = np.int64(256) * x + np.int64(128), np.int64(256) * y + np.int64(128)
    return [np.int64(dx) * (py - np.int64(ya)) - np.int64(dy) * (px - np.int64(xa)) for dx, dy, xa, ya, _ in edges]


def _barycentrics(E, A):
    fa = np.array(A, np.int64).astype(F)
    return [e.astype(F) / fa for e in E]


def _z(l, z):
    return ((l[0] * z[0] + l[1] * z[1]) + l[2] * z[2]) + F(0.0)


def rasterize(meshes, draws, view, coverage_counts=None):
    """The whole call. ``coverage_counts``: an optional (rows, W) int array that receives, per pixel, how many
    triangles' coverage tests it passed (before the depth range): the top-left rule's self-check."""
    W, H = int(view.width), int(view.height)
    r0 = int(view.row_begin)
    r1 = H if view.row_end is None else int(view.row_end)
    rows = r1 - r0
    vis = np.full((rows, W), EMPTY, np.uint64)
    stats = dict.fromkeys(STAT_NAMES, 0)
    setups = {}  # prim -> (vertex stage of its draw, its three vertex indices in setup order, A, material)
    prim = 0
    with np.errstate(all="ignore"):
        for dr in draws:
            mesh = meshes[dr.mesh]
            vs = vertex_stage(mesh.vertices, dr, view)
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
                x0, x1 = max((min(X) - 128 + 255) >> 8, 0), min((max(X) - 128) >> 8, W - 1)
                y0, y1 = max((min(Y) - 128 + 255) >> 8, r0), min((max(Y) - 128) >> 8, r1 - 1)
                if x0 > x1 or y0 > y1:
                    continue
                y, x = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64),
                                   indexing="ij")
                edges = _edges(X, Y)
                E = _edge_values(edges, x, y)
                cov = np.ones(x.shape, bool)
                for e, (_, _, _, _, top_left) in zip(E, edges):
                    cov &= (e > 0) | ((e == 0) & top_left)
                if coverage_counts is not None:
                    coverage_counts[y0 - r0:y1 + 1 - r0, x0:x1 + 1] += cov
                l = _barycentrics(E, A)
                z = _z(l, [vs["z"][k] for k in i]).astype(F)
                frag = cov & (z >= F(0)) & (z < F(1))  # NaN: no fragment
                stats["fragments"] += int(frag.sum())
                key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
                sub = vis[y0 - r0:y1 + 1 - r0, x0:x1 + 1]
                sub[frag] = np.minimum(sub[frag], key[frag])

        planes = np.zeros((14, rows, W), F)
        material = np.full((rows, W), NONE, np.uint16)
        depth = np.ones((rows, W), F)
        yy, xx = np.meshgrid(np.arange(r0, r1, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
        # step 9: the background everywhere, then the winners over it
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
        prims = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
        for t in np.unique(prims[won]).tolist():
            vs, i, A, mat = setups[t]
            m = won & (prims == t)
            x, y = xx[m], yy[m]
            E = _edge_values(_edges([int(vs["X"][k]) for k in i], [int(vs["Y"][k]) for k in i]), x, y)
            l = _barycentrics(E, A)
            depth[m] = _z(l, [vs["z"][k] for k in i])
            p = [l[k] * vs["rw"][i[k]] for k in range(3)]
            s = (p[0] + p[1]) + p[2]
            q = [p[k] / s for k in range(3)]
            for k in range(14):
                a = vs["a"][k]
                planes[k][m] = (q[0] * a[i[0]] + q[1] * a[i[1]]) + q[2] * a[i[2]]
            material[m] = mat
    assert np.array_equal(depth[won].view(np.uint32), (vis[won] >> np.uint64(32)).astype(np.uint32))
    return planes, material, depth, stats
