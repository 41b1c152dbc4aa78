"""The numpy restatement of near-plane clipping (tests/raster_clip_reference.py) against the
rules it encodes, on the scenes of tests/raster_clip_cases.py and tests/raster_cases.py. No GPU."""
import numpy as np
import pytest

import raster_cases as C
import raster_clip_cases as CC
import raster_clip_reference as CR
import raster_reference as R

FRAMES = list(CC.FRAMES.items())
_cache = {}


def clipped(module, name, frame):
    """(case, flagged restatement, coverage counts, details) of one case, computed once and shared."""
    key = (module.__name__, name, frame)
    if key not in _cache:
        W, H = module.FRAMES[frame]
        scene = module.case(name, W, H)
        counts, details = np.zeros((H, W), np.int64), {}
        _cache[key] = (scene, CR.rasterize(*scene, coverage_counts=counts, details=details), counts, details)
    return _cache[key]


def bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def any_vertex_outside(meshes, draws, view):
    """Is PosH.z of some vertex a drawn triangle uses not >= 0?"""
    for dr in draws:
        mesh = meshes[dr.mesh]
        count = mesh.indices.size - dr.first_index if dr.index_count is None else dr.index_count
        used = np.unique(mesh.indices[dr.first_index:dr.first_index + count])
        if not (CR.clip_space(mesh.vertices, dr, view)[2, used] >= 0).all():
            return True
    return False


def identity_holds(stats, clip, details):
    """triangles + clip_pieces - clipped_near = drawn + backface_culled + zero_area + skipped_near + skipped_guard_band."""
    return (stats["triangles"] + clip["clip_pieces"] - clip["clipped_near"] ==
            details["drawn"] + stats["backface_culled"] + stats["zero_area"] + stats["skipped_near"] +
            stats["skipped_guard_band"])


@pytest.mark.parametrize("frame", list(C.FRAMES))
@pytest.mark.parametrize("module,name", [(CC, "overview")] + [(C, n) for n in C.CASES])
def test_flagged_equals_unflagged_where_no_vertex_is_outside(module, name, frame):
    """Case (j) and every case of raster_cases.py: with no vertex in front of z = 0 the flagged restatement equals
    raster_reference.rasterize bit for bit in all 16 planes and in the statistics, and clips nothing. (A case with
    such a vertex -- near_and_guard, depth_range, nan_inf -- is cut where the unflagged call skips the triangle or
    cuts per fragment, so its planes legitimately differ; there the counter identity is what is held.)"""
    scene, (planes, ids, depth, stats, clip), _, details = clipped(module, name, frame)
    assert identity_holds(stats, clip, details)
    if any_vertex_outside(*scene):
        assert name in ("near_and_guard", "depth_range", "nan_inf"), name
        assert clip["clipped_near"] > 0 or stats["skipped_near"] > 0
        return
    uplanes, uids, udepth, ustats = R.rasterize(*scene)
    assert bits_equal(planes, uplanes) and np.array_equal(ids, uids) and bits_equal(depth, udepth)
    assert stats == ustats and clip == dict.fromkeys(CR.CLIP_STAT_NAMES, 0)


@pytest.mark.parametrize("frame", list(CC.FRAMES))
@pytest.mark.parametrize("name", [n for n in CC.CASES if n != "overview"])
def test_counter_identity_and_what_the_cases_exercise(name, frame):
    scene, (planes, ids, depth, stats, clip), _, details = clipped(CC, name, frame)
    assert identity_holds(stats, clip, details)
    assert clip["clipped_near"] <= clip["clip_pieces"] <= 2 * clip["clipped_near"]
    unflagged = R.rasterize(*scene)
    if name == "floor_quad":  # today's behaviour: both triangles dropped, the frame all background
        assert unflagged[3]["skipped_near"] == 2 and (unflagged[1] == R.NONE).all()
        assert clip == {"clipped_near": 2, "clip_pieces": 3} and (ids == 1).mean() > 0.15
    elif name.startswith("single_"):
        n = int(name[8])
        assert clip == {"clipped_near": 1, "clip_pieces": n}
        assert unflagged[3]["skipped_near"] == 1 and (unflagged[1] == R.NONE).all()
        if name.endswith("cull0_back"):
            assert stats["backface_culled"] == n and (ids == R.NONE).all()  # culling is per piece
        else:
            assert details["drawn"] == n and (ids == 3).any()
    elif name == "zero_z":
        m, d, v = scene
        z = CR.clip_space(m[0].vertices, d[0], v)[2]
        assert z[0] == 0 and not np.signbit(z[0]) and z[3] == 0 and np.signbit(z[3])  # +0.0f and -0.0f exactly
        assert np.signbit(z[[7, 9]]).all() and (z[[6, 7, 9]] == 0).all()
        # -0.0f is inside: the triangle (+0, -0, inside) is not clipped, the other three are
        assert clip["clipped_near"] == 3 and stats["skipped_near"] == 0
    elif name == "behind":
        assert stats["skipped_near"] == 1 and clip == {"clipped_near": 0, "clip_pieces": 0} and details["drawn"] == 1
    elif name == "nan_vertex":  # the NaN vertex is outside; its crossings are NaN, so both pieces are skipped near
        assert clip == {"clipped_near": 2, "clip_pieces": 4} and stats["skipped_near"] == 2
        assert stats["skipped_guard_band"] == 0 and details["drawn"] == 3
    elif name == "tiny_and_floor":  # the two tiny triangles' pieces have boxes of at most 64 pixels
        assert (ids == 7).any() and (ids == 1).any()
        tiny = [v for v in details["new_vertices"] if v.vs["a"].shape[1] == 6]
        assert len(tiny) == 5  # n = 1: two crossings; n = 2: three, one of them twice
        for group in (tiny[:2], tiny[2:]):  # each triangle's crossings lie within 8 pixels of each other
            xs, ys = [v.X for v in group], [v.Y for v in group]
            assert max(xs) - min(xs) < 8 * 256 and max(ys) - min(ys) < 8 * 256
    elif name == "floor_sphere_floor":  # equal z: the first floor keeps every floor pixel, clipped or not
        assert (ids == 0).any() and (ids == 1).any() and not (ids == 2).any()
        assert (ids == 0).sum() > (unflagged[1] == 0).sum()
    elif name == "inside_sphere":
        assert (ids == 8).all() and (unflagged[1] == R.NONE).any()


@pytest.mark.parametrize("frame,size", FRAMES)
def test_inside_a_sphere_every_pixel_passes_exactly_one_piece(frame, size):
    """(i): the clipped sphere around the eye is closed on the screen: every pixel centre passes the coverage test of
    exactly one triangle or piece -- crossing edges shared by two triangles are cut into the identical vertex."""
    _, _, counts, _ = clipped(CC, "inside_sphere", frame)
    assert (counts == 1).all(), np.argwhere(counts != 1)[:8].tolist()


@pytest.mark.parametrize("frame,size", FRAMES)
def test_floor_grid_pixels_pass_exactly_one_piece(frame, size):
    """(b): a pixel whose centre's ray meets the floor rectangle in front of the near plane passes exactly one
    piece's coverage test, one whose ray misses it none. Pixels within 1e-3 (relative) of the rectangle's rim are
    left to either side: the vertices are snapped to 1/256 pixel."""
    W, H = size
    (_, _, view), _, counts, _ = clipped(CC, "floor_grid", frame)
    hit, t = floor_hits(view, W, H)
    x, z = hit[..., 0], hit[..., 2]
    ahead = t > 0
    inside = ahead & (np.abs(x) < 3.0 * (1 - 1e-3)) & (z > -4.0 + 0.012) & (z < 8.0 * (1 - 1e-3))
    outside = ~ahead | (np.abs(x) > 3.0 * (1 + 1e-3)) | (z < -4.0 - 0.012) | (z > 8.0 * (1 + 1e-3))
    assert inside.sum() > 0.1 * W * H
    assert (counts <= 1).all() and (counts[inside] == 1).all() and (counts[outside] == 0).all()


def floor_hits(view, W, H):
    """Where the ray through each pixel centre meets the plane y = FLOOR_Y (float64), and its parameter."""
    eye, Fw, Rt, Up = (np.asarray(v, np.float64) for v in (view.eye, view.bg_forward, view.bg_right, view.bg_up))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sx, sy = (2 * xx + 1) / W - 1, 1 - (2 * yy + 1) / H
    d = Fw + sx[..., None] * Rt + sy[..., None] * Up
    with np.errstate(all="ignore"):
        t = (CC.FLOOR_Y - eye[1]) / d[..., 1]
        return eye + t[..., None] * d, t


# The restatement's largest error against the analytic ray-plane hit on case (a), measured on the CPU at the two
# frames: PosW.x 9.41e-4 (70x37) and 7.65e-5 (256x64), PosW.z 2.35e-3 (70x37) and 5.29e-4 (256x64) -- the vertices'
# snap to 1/256 pixel, seen through the perspective near the horizon (|z| up to 6.5). The bound is 4 x the larger.
POS_X_BOUND, POS_Z_BOUND = 4 * 9.41e-4, 4 * 2.35e-3


@pytest.mark.parametrize("frame,size", FRAMES)
def test_floor_quad_positions(frame, size):
    """(a): every new vertex's PosW.y is exactly -1.0f (a + t (b - a) with b == a), and the PosW.y plane is -1 on
    floor pixels to within 4 x 2^-24: step 8 gives -(q0 + q1 + q2) with each q rounded once and two rounded sums, so
    not always -1.0f to the bit (the restatement gives -1 - 2^-23 to -1 + 2^-23 here, as it does for an unclipped
    floor). PosW.xz is within the bound above of the analytic ray-plane hit."""
    W, H = size
    (_, _, view), (planes, ids, _, _, _), _, details = clipped(CC, "floor_quad", frame)
    assert len(details["new_vertices"]) == 5  # n = 1: two crossings; n = 2: three, one of them twice
    for v in details["new_vertices"]:
        assert v.attribute(1) == np.float32(-1.0)
    fl = ids == 1
    err_y = np.abs(planes[1][fl].astype(np.float64) + 1.0).max()
    hit, _ = floor_hits(view, W, H)
    err_x, err_z = np.abs(planes[0] - hit[..., 0])[fl].max(), np.abs(planes[2] - hit[..., 2])[fl].max()
    print(f"floor_quad {frame}: |PosW.y + 1| {err_y:.3g}, PosW.x err {err_x:.3g}, PosW.z err {err_z:.3g}")
    assert err_y <= 4 * 2.0 ** -24
    assert err_x <= POS_X_BOUND and err_z <= POS_Z_BOUND


@pytest.mark.parametrize("frame", list(CC.FRAMES))
@pytest.mark.parametrize("n", (1, 2))
def test_rotations_of_one_triangle_cover_the_same_pixels(n, frame):
    """(c): the three rotations of a triangle's indices give the same crossings (each is computed from its inside to
    its outside vertex whatever the index order), so the same pixel set; so does the back-facing order under cull 1
    (1 and 2 exchanged per piece)."""
    sets = {}
    for r in (0, 1, 2):
        for cull, face in ((0, "front"), (1, "front"), (1, "back")):
            _, (_, ids, _, _, _), _, _ = clipped(CC, f"single_n{n}_rot{r}_cull{cull}_{face}", frame)
            sets[(r, cull, face)] = ids != R.NONE
    first = sets[(0, 0, "front")]
    assert first.sum() > 100
    for key, got in sets.items():
        assert np.array_equal(got, first), key
