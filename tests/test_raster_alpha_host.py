"""The numpy restatement of the rasteriser's alpha test (tests/raster_alpha_reference.py)
against the rules it encodes, on the scenes of tests/raster_alpha_cases.py. No GPU."""
import numpy as np
import pytest

import raster_alpha_cases as AC
import raster_alpha_reference as AR
import raster_clip_reference as CR
import raster_reference as R
import resolve_reference as RR

F = np.float32
_cache = {}


def restated(name, frame, alpha_test=True):
    """(scene, restatement, details) of one case, computed once and shared."""
    key = (name, frame, alpha_test)
    if key not in _cache:
        W, H = AC.FRAMES[frame]
        scene = AC.case(name, W, H)
        details = {}
        _cache[key] = (scene, AR.rasterize(*scene, alpha_test=alpha_test, details=details), details)
    return _cache[key]


def bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_frame(a, b):
    return bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and bits_equal(a[2], b[2])


def older_restatement(scene):
    """The scene without the flag through the restatements the alpha one is built on."""
    m, d, v, _, _, clip_near = scene
    if clip_near:
        return CR.rasterize(m, d, v)
    return R.rasterize(m, d, v) + (dict.fromkeys(CR.CLIP_STAT_NAMES, 0),)


@pytest.mark.parametrize("frame", list(AC.FRAMES))
@pytest.mark.parametrize("name", AC.CASES)
def test_without_the_flag_it_is_the_older_restatement(name, frame):
    """alpha_test = False walks the same code and equals raster_reference / raster_clip_reference bit for bit, in all 16
    planes and the eight old counters, with both new counters 0."""
    scene, got, _ = restated(name, frame, alpha_test=False)
    want = older_restatement(scene)
    assert same_frame(got, want) and got[3] == want[3] and got[4] == want[4]
    assert got[5] == {"alpha_tested": 0, "alpha_discarded": 0}


@pytest.mark.parametrize("frame", list(AC.FRAMES))
@pytest.mark.parametrize("name", AC.CASES)
def test_counter_identities(name, frame):
    """fragments keeps counting discarded fragments: visibility updates = fragments - alpha_discarded; the old
    counters do not depend on the flag; round 11's identity with pieces holds."""
    _, (_, _, _, stats, clip, alpha), details = restated(name, frame)
    _, unflagged, udetails = restated(name, frame, alpha_test=False)
    assert details["updates"] == stats["fragments"] - alpha["alpha_discarded"]
    assert 0 <= alpha["alpha_discarded"] <= alpha["alpha_tested"] <= stats["fragments"]
    assert stats == unflagged[3] and clip == unflagged[4] and details["drawn"] == udetails["drawn"]
    assert (stats["triangles"] + clip["clip_pieces"] - clip["clipped_near"] ==
            details["drawn"] + stats["backface_culled"] + stats["zero_area"] + stats["skipped_near"] +
            stats["skipped_guard_band"])
    if name == "clip_floor_sphere":
        assert clip["clipped_near"] > 0 and clip["clip_pieces"] > clip["clipped_near"]  # n = 1 and n = 2 both occur


@pytest.mark.parametrize("frame", list(AC.FRAMES))
@pytest.mark.parametrize("name", AC.CUTOUT_CASES)
def test_no_case_passes_vacuously(name, frame):
    """Every case but the all-or-nothing ones discards some tested fragments and keeps others, and some pixel's winner
    differs from the unflagged restatement's."""
    _, (planes, ids, depth, _, _, alpha), _ = restated(name, frame)
    _, unflagged, _ = restated(name, frame, alpha_test=False)
    assert alpha["alpha_discarded"] > 0 and alpha["alpha_tested"] > alpha["alpha_discarded"], alpha
    assert (ids != unflagged[1]).any() or not bits_equal(depth, unflagged[2])
    assert not same_frame((planes, ids, depth), unflagged)


@pytest.mark.parametrize("frame", list(AC.FRAMES))
def test_the_two_checker_cases_take_the_two_coverage_paths(frame):
    """checker_small: every triangle of the tested quad has a box of at most 64 pixels (rasterised by its setup
    lane); checker_large: both have more (the large-triangle kernel). The boxes are those of step 4 on the snapped
    vertices."""
    for name, small in (("checker_small", True), ("checker_large", False)):
        (m, d, v, _, _, _), _, _ = restated(name, frame)
        vs = R.vertex_stage(m[0].vertices, d[0], v)
        for tri in m[0].indices.reshape(-1, 3):
            X, Y = vs["X"][tri], vs["Y"][tri]
            nx = min((X.max() - 128) >> 8, v.width - 1) - max((X.min() - 128 + 255) >> 8, 0) + 1
            ny = min((Y.max() - 128) >> 8, v.height - 1) - max((Y.min() - 128 + 255) >> 8, 0) + 1
            assert (nx * ny <= 64) == small, (name, nx, ny)


@pytest.mark.parametrize("frame", list(AC.FRAMES))
def test_all_255_and_no_tested_material_equal_the_unflagged_restatement(frame):
    for name in ("all_255", "no_tested"):
        _, got, _ = restated(name, frame)
        _, want, _ = restated(name, frame, alpha_test=False)
        assert same_frame(got, want) and got[3] == want[3] and got[4] == want[4], name
        assert got[5]["alpha_discarded"] == 0
    assert restated("all_255", frame)[1][5]["alpha_tested"] > 0
    assert restated("no_tested", frame)[1][5] == {"alpha_tested": 0, "alpha_discarded": 0}
    # the opacity-0 material of no_tested is in front and visible: a constant opacity is never a test
    assert (restated("no_tested", frame)[1][1] == 0).sum() > 100


@pytest.mark.parametrize("frame", list(AC.FRAMES))
def test_all_zero_is_the_background_of_a_call_without_draws(frame):
    (m, _, v, mats, texs, clip_near), got, _ = restated("all_zero", frame)
    empty = AR.rasterize(m, [], v, mats, texs, clip_near)
    assert same_frame(got, empty) and (got[1] == R.NONE).all() and (got[2] == F(1.0)).all()
    assert got[5]["alpha_tested"] == got[5]["alpha_discarded"] == got[3]["fragments"] > 0


def test_the_threshold_lies_between_bytes_25_and_26():
    """o - 0.1f < 0.0f with o = (float)byte / 255.0f: bytes 0..25 are discarded, 26..255 kept -- in the decision
    function, and in the case that maps byte 16 j + i to pixel (3 + i, 2 + j)."""
    kill = AR.discarded(RR.decode_unorm8(np.arange(256, dtype=np.uint8)))
    assert kill[:26].all() and not kill[26:].any()
    for frame in AC.FRAMES:
        _, (_, ids, _, _, _, alpha), _ = restated("threshold", frame)
        byte = np.arange(256).reshape(16, 16)
        assert np.array_equal(ids[2:18, 3:19] == 0, byte >= 26)
        assert alpha == {"alpha_tested": 256, "alpha_discarded": 26}


@pytest.mark.parametrize("frame", list(AC.FRAMES))
def test_complementary_checkerboards_cover_the_quad_exactly_once(frame):
    """Equal depth everywhere: the earlier draw keeps what it keeps, the later one wins exactly where the earlier one
    is discarded; together they cover every pixel of the quad, neither draw's kept set overlapping the other's."""
    scene, (_, ids, _, stats, _, alpha), _ = restated("complementary", frame)
    _, (_, uids, _, _, _, _), _ = restated("complementary", frame, alpha_test=False)
    quad = uids != R.NONE
    assert (uids[quad] == 0).all()  # unflagged: the earlier draw everywhere
    assert np.array_equal(ids != R.NONE, quad) and set(np.unique(ids[quad]).tolist()) == {0, 1}
    assert stats["fragments"] == 2 * quad.sum() == alpha["alpha_tested"]
    assert alpha["alpha_discarded"] == quad.sum()  # every pixel discards exactly one of its two fragments
    m, d, v, mats, texs, clip_near = scene
    first = AR.rasterize(m, d[:1], v, mats, texs, clip_near)[1] != R.NONE
    second = AR.rasterize(m, d[1:], v, mats, texs, clip_near)[1] != R.NONE
    assert not (first & second).any() and np.array_equal(first | second, quad)
    assert np.array_equal(ids == 0, first) and np.array_equal(ids == 1, second)


@pytest.mark.parametrize("name", ["checker_large", "checker_small"])
@pytest.mark.parametrize("frame", list(AC.FRAMES))
def test_visible_set_is_the_unflagged_one_filtered_by_a_texel_lookup(name, frame):
    """Where the tested quad is front-most without the flag, it stays visible exactly where a direct lookup of the
    opacity texture at the unflagged planes' TexCoord passes the test: the test sees the TexCoord the resolve writes."""
    (_, _, _, _, texs, _), (planes, ids, _, _, _, _), _ = restated(name, frame)
    _, (uplanes, uids, _, _, _, _), _ = restated(name, frame, alpha_test=False)
    front = uids == 0
    _, o = AR.opacity_at(RR._texture(texs[0]), uplanes[12][front], uplanes[13][front])
    keep = ~AR.discarded(o)
    assert keep.any() and not keep.all()
    assert np.array_equal(ids[front] == 0, keep)
    for k in range(14):  # a kept pixel is the unflagged pixel
        assert bits_equal(planes[k][front][keep], uplanes[k][front][keep])
    assert set(np.unique(ids[front][~keep]).tolist()) == {1, R.NONE}  # behind a hole: the opaque quad, or the background


@pytest.mark.parametrize("name,frame", [("checker_small", "70x37"), ("clip_floor_sphere", "256x64")])
def test_a_band_equals_the_same_rows_of_the_full_frame(name, frame):
    scene, full, _ = restated(name, frame)
    m, d, v, mats, texs, clip_near = scene
    H = v.height
    total = dict.fromkeys(AR.ALPHA_STAT_NAMES, 0)
    for r0, r1 in ((0, 5), (5, 6), (6, H - 9), (H - 9, H)):
        band = AR.rasterize(m, d, v.rows(r0, r1), mats, texs, clip_near)
        assert same_frame(band, (full[0][:, r0:r1], full[1][r0:r1], full[2][r0:r1])), (r0, r1)
        for k in total:
            total[k] += band[5][k]
    assert total == full[5]  # a fragment belongs to one band


@pytest.mark.parametrize("frame", list(AC.FRAMES))
@pytest.mark.parametrize("name", AC.CUTOUT_CASES)
def test_every_visible_tested_pixel_resolves_to_a_passing_opacity(name, frame):
    """The tie to the rest of the pipeline: the opacity the material resolve writes for a visible pixel of a tested
    draw satisfies o - 0.1f >= 0, so a shading pass with PBR_FLAG_ALPHA_TEST discards none of them."""
    (_, _, _, mats, texs, _), (planes, ids, _, _, _, _), _ = restated(name, frame)
    _, opacity, _ = RR.resolve(planes, ids, mats, texs, RR.POINT)
    is_tested = np.zeros(ids.shape, bool)
    for k, m in enumerate(mats):
        if int(m.flags) & AC.ALPHA:
            is_tested |= ids == k
    assert is_tested.any() and not AR.discarded(opacity[is_tested]).any()
