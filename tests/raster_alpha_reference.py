"""The rasteriser's alpha test (pbr_rasterize_flags with PBR_RASTER_ALPHA_TEST, csrc/raster.h)
restated in numpy on top of tests/raster_reference.py and tests/raster_clip_reference.py: int64 edge functions, float32
everywhere else, one numpy operation per specified operation. A helper, not a test: tests/test_raster_alpha_host.py
checks the restatement against the rules it encodes, tests/test_gpu_raster_alpha.py holds the device to it bit for bit.

    rasterize(meshes, draws, view, materials, textures, clip_near=False, alpha_test=True)
        -> (planes (14, rows, W) float32, material (rows, W) uint16, depth (rows, W) float32,
            stats dict, clip stats dict, alpha stats dict)

``materials`` a list of renderer.Material, ``textures`` a list of uint8 arrays, as ShadingContext.set_materials takes
them. With ``alpha_test`` False no fragment is tested: the unflagged (or only clipping) call through the same code, which
tests/test_raster_alpha_host.py holds equal to raster_reference.rasterize / raster_clip_reference.rasterize."""
import numpy as np

import raster_clip_reference as CR
import raster_reference as R
import resolve_reference as RR
from physically_based_renderer_amd import _native as N

F = R.F
ALPHA_STAT_NAMES = ("alpha_tested", "alpha_discarded")
THRESHOLD = F(0.1)


def tested_texture(draw, materials, textures):
    """The opacity texture (h, w, c) uint8 the fragments of `draw` are tested against, or None: the draw's material id
    is at or past the table's count, or its record has no PBR_MAT_ALPHA_TEST."""
    if not 0 <= int(draw.material) < len(materials):
        return None
    m = materials[int(draw.material)]
    if not int(m.flags) & N.PBR_MAT_ALPHA_TEST:
        return None
    return RR._texture(textures[int(m.tex[5])])


def opacity_at(tex, u, v):
    """The resolve's point-wrap tap of the red byte at float32 (u, v) and its decode: (byte, (float)byte / 255.0f)."""
    h, w = tex.shape[0], tex.shape[1]
    with np.errstate(all="ignore"):
        tx = RR.wrap_index(np.floor(u * F(w)), w)
        ty = RR.wrap_index(np.floor(v * F(h)), h)
    r8 = tex[ty, tx, 0]
    return r8, RR.decode_unorm8(r8)


def discarded(o):
    """clip(o - 0.1f): discarded iff o - 0.1f < 0.0f."""
    return (o - THRESHOLD) < F(0.0)


def fragment_uv(p, l):
    """Step 8's TexCoord of the fragments with barycentrics l of the set-up piece p: p_i = l_i * rw_i,
    s = (p0 + p1) + p2, q_i = p_i / s, u = (q0 u0 + q1 u1) + q2 u2."""
    pr = [l[k] * p[k].rw for k in range(3)]
    s = (pr[0] + pr[1]) + pr[2]
    q = [pr[k] / s for k in range(3)]
    u = (q[0] * p[0].attribute(12) + q[1] * p[1].attribute(12)) + q[2] * p[2].attribute(12)
    v = (q[0] * p[0].attribute(13) + q[1] * p[1].attribute(13)) + q[2] * p[2].attribute(13)
    return u.astype(F), v.astype(F)


def rasterize(meshes, draws, view, materials, textures, clip_near=False, alpha_test=True, details=None):
    """The whole call. ``details``: an optional dict that receives ``drawn``, the number of triangles and pieces that
    reached coverage, and ``updates``, the number of visibility updates issued."""
    W, H = int(view.width), int(view.height)
    r0 = int(view.row_begin)
    r1 = H if view.row_end is None else int(view.row_end)
    rows = r1 - r0
    vis = np.full((rows, W), R.EMPTY, np.uint64)
    stats = dict.fromkeys(R.STAT_NAMES, 0)
    clip = dict.fromkeys(CR.CLIP_STAT_NAMES, 0)
    alpha = dict.fromkeys(ALPHA_STAT_NAMES, 0)
    setups = {}  # prim -> [(piece in setup order, A, material)] in piece order
    updates = 0
    prim = 0
    with np.errstate(all="ignore"):
        for dr in draws:
            mesh = meshes[dr.mesh]
            vs = R.vertex_stage(mesh.vertices, dr, view)
            ph = CR.clip_space(mesh.vertices, dr, view)
            tex = tested_texture(dr, materials, textures) if alpha_test else None
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
                else:  # the submitted triangle, whole: the w > 0 rule below skips it when a vertex is behind
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
                    cov, l, z = CR._coverage(p, A, x, y)
                    frag = cov & (z >= F(0)) & (z < F(1))  # NaN: no fragment
                    stats["fragments"] += int(frag.sum())
                    if tex is not None:  # step 6a
                        u, v = fragment_uv(p, l)
                        _, o = opacity_at(tex, u, v)
                        kill = frag & discarded(o)
                        alpha["alpha_tested"] += int(frag.sum())
                        alpha["alpha_discarded"] += int(kill.sum())
                        frag = frag & ~kill
                    updates += int(frag.sum())
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
            for p, A, mat in setups[t]:  # steps 8 and 2a.8, unchanged: the lowest-numbered piece that made the key
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
    if details is not None:
        details["drawn"] = sum(len(v) for v in setups.values())
        details["updates"] = updates
    assert np.array_equal(resolved, won)
    assert np.array_equal(depth[won].view(np.uint32), zbits[won])
    return planes, material, depth, stats, clip, alpha
