"""The numpy restatements of the rasteriser against the float64 geometric truth of tests/raster_truth.py (DESIGN.md
§12, "Distance of the rule set from exact geometry"); no device needed. tests/test_gpu_raster_truth.py holds the device
planes to the same truth without going through the restatements.

At every sure pixel the restatement must name the truth's winner (material; for layers also prim_out), keep the 14
planes and the depth inside the truth's five-point interval widened by tau_k = 32 * 2^-24 * S_k, and give the truth's
background where nothing is drawn. The caps (at most 2% of the frame unsure, at least 95% of the drawn pixels checked)
are conditions on the scene, asserted per case and frame. Scenes built to put edges through pixel centres or to tie on
depth -- fan, split_quad, centres_and_corners, coplanar_*, equal_z, floor_sphere_floor -- are not run: the truth
abstains on them by construction, and the exactly-once tests of the bit-for-bit suites own those rules. `overview` is
looked at from a camera moved off the scene's plane of symmetry and with coarser spheres (raster_truth.OVERVIEW_NUDGE):
as tests/raster_clip_cases.py builds it, facet edges run through pixel centres and the facets at 70x37 are smaller than
a pixel, so that 14% of its drawn pixels are unsure.

What this test cannot see: a snap that truncates instead of rounding half to even moves a vertex by less than DELTA and
stays inside the bound; the bit-for-bit tests own that rule."""
import numpy as np
import pytest

import raster_alpha_reference as AR
import raster_cases as C
import raster_clip_cases as CC
import raster_clip_reference as CR
import raster_layer_reference as LR
import raster_reference as R
import raster_truth as RT

F = np.float32



def run_flat(family, name, frame, alpha_test=True):
    """One plain, clipped, alpha-tested or soup case: (report, failures)."""
    m, d, v, clip_near, mats, texs, _ = RT.scene(family, name, frame)
    T = RT.truth(family, name, frame)
    what = f"{family} {name} {frame}"
    clip = alpha = None
    if family == "alpha":
        planes, mat, depth, stats, clip, alpha = AR.rasterize(m, d, v, mats, texs, clip_near)
        clip = clip if clip_near else None
    elif clip_near:
        planes, mat, depth, stats, clip = CR.rasterize(m, d, v)
    else:
        planes, mat, depth, stats = R.rasterize(m, d, v)
    rep = T.check(T.winners(), planes, mat, depth, what=what)
    fails = rep.failures + rep.caps(what) + RT.counter_failures(T, stats, clip, alpha, what)
    if T.marginal and (family, name) not in RT.MARGINAL_ALLOWED:
        fails.append(f"{what}: {T.marginal} triangles of marginal area")
    print(rep.line(what))
    return rep, fails


def run_layers(name, frame):
    """One layer case, the restatement's sequence down to the empty layer: (reports, failures)."""
    m, d, v, clip_near, _, _, opaque = RT.scene("layer", name, frame)
    T = RT.truth("layer", name, frame)
    what = f"layer {name} {frame}"
    fails, reps = [], []
    p0, m0, d0, s0, c0, _ = AR.rasterize(m, opaque, v, [], [], clip_near, alpha_test=False)
    if opaque:  # the incoming depth is itself a rasterisation: held to the truth of the opaque draws
        T0 = RT.Truth(m, opaque, v, clip_near)
        rep = T0.check(T0.winners(), p0, m0, d0, what=what + " opaque")
        fails += rep.failures + RT.counter_failures(T0, s0, c0 if clip_near else None, None, what + " opaque")
    layers = LR.peel(m, d, v, d0, clip_near)
    sure, wins = T.layers(d0)
    if len(wins) > len(layers):
        fails.append(f"{what}: {len(layers)} layers, the truth has {len(wins)}")
    prev = d0
    for k, L in enumerate(layers):
        rep = T.check(wins[min(k, len(wins) - 1)], L.planes, L.material, L.depth, background_depth=prev, prim=L.prim,
                      what=f"{what} layer {k}")
        fails += rep.failures + RT.counter_failures(T, L.stats, L.clip if clip_near else None, None, f"{what} layer {k}")
        reps.append(rep)
        prev = L.depth
    fails += RT.sequence_caps(what, sure, reps)
    if T.marginal and ("layer", name) not in RT.MARGINAL_ALLOWED:
        fails.append(f"{what}: {T.marginal} triangles of marginal area")
    return reps, fails


def both_frames(run, frames=RT.FRAMES):
    fails = []
    for frame in frames:
        fails += run(frame)[1]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", RT.PLAIN_CASES)
def test_plain_restatement_inside_the_truth(name):
    both_frames(lambda frame: run_flat("plain", name, frame))


@pytest.mark.parametrize("name", RT.CLIP_CASES + CC.SINGLE_CASES)
def test_clip_restatement_inside_the_truth(name):
    both_frames(lambda frame: run_flat("clip", name, frame))


@pytest.mark.parametrize("name", RT.ALPHA_CASES)
def test_alpha_restatement_inside_the_truth(name):
    """The visible set is the material plane's: a discarded fragment shows what lies behind it."""
    both_frames(lambda frame: run_flat("alpha", name, frame))


@pytest.mark.parametrize("name", RT.LAYER_CASES)
def test_layer_restatement_inside_the_truth(name):
    both_frames(lambda frame: run_layers(name, frame))


@pytest.mark.parametrize("seed", RT.SOUP_SEEDS)
def test_soup_restatement_inside_the_truth(seed):
    both_frames(lambda frame: run_flat("soup", str(seed), frame), RT.SOUP_FRAMES)


def test_alpha_cases_discard_and_keep_certainly():
    """The alpha scenes are decided by the truth, not abstained on: each has certainly discarded and certainly kept
    fragments, and the winners differ from the truth of the same call without the test."""
    for name in RT.ALPHA_CASES:
        T, U = RT.truth("alpha", name, "70x37"), RT.truth("alpha", name, "70x37", False)
        assert T.alpha_discarded_lo > 0 and T.alpha_tested_lo > T.alpha_discarded_hi, name
        a, b = T.winners(), U.winners()
        assert ((a != b) & (a != RT.UNSURE) & (b != RT.UNSURE)).any(), name


# -- by hand ---------------------------------------------------------------------------------------------------------

# One perspective triangle in a 16 x 12 frame under raster_cases.PERSP, (x px, y px, w): clockwise with y down (the
# screen area (10.5 - 2.5)(10.5 - 1.5) - (5.5 - 2.5)(5.5 - 1.5) = 72 - 12 = 60 > 0), so front facing.
HAND = [(2.5, 1.5, 1.0), (10.5, 5.5, 3.0), (5.5, 10.5, 2.0)]


def hand_truth(points=HAND, cull=0):
    m, d = C.one_draw(points, 16, 12, 77, cull=cull)
    return m, d, C.screen_view(16, 12), RT.Truth(m, d, C.screen_view(16, 12))


def test_facing_sign_on_a_hand_checked_triangle():
    m, d, v, T = hand_truth()
    assert T.tri[0] is not None and T.tri[0]["front"] and T.counters["backface_culled"] == 0
    m, d, v, T = hand_truth([HAND[0], HAND[2], HAND[1]])
    assert T.tri[0] is None and T.counters["backface_culled"] == 1
    m, d, v, T = hand_truth([HAND[0], HAND[2], HAND[1]], cull=1)
    assert T.tri[0] is not None and not T.tri[0]["front"]
    assert R.rasterize(*hand_truth()[:3])[3]["backface_culled"] == 0  # the rules' A > 0 agrees


def test_two_pixels_worked_by_hand():
    """The midpoint of edge 0-1 in clip space is (h_0 + h_1) / 2: it lands at ((2.5 * 1 + 10.5 * 3) / 4,
    (1.5 * 1 + 5.5 * 3) / 4) = (8.5, 4.5), the centre of pixel (8, 4), with q = (1/2, 1/2, 0): the attribute there is
    the plain mean of the two vertices', not the screen-space mix (1/4, 3/4). The centroid (h_0 + h_1 + h_2) / 3 lands
    at ((2.5 + 31.5 + 11) / 6, (1.5 + 16.5 + 21) / 6) = (7.5, 6.5), the centre of pixel (7, 6), with q = 1/3 each.
    Under PERSP PosH.z = (w - 0.1) * 100 / 99.9, so z = (sum w - 0.1 n) / sum w * 100 / 99.9: (4 - 0.2) / 4 * 1.001001 =
    0.950951 at the midpoint, (6 - 0.3) / 6 * 1.001001 = 0.950951 at the centroid."""
    m, d, v, T = hand_truth()
    a = m[0].vertices.astype(np.float64)
    q, out, z = T.at(0, 8.5, 4.5)
    assert np.allclose(q, (0.5, 0.5, 0.0), atol=1e-6)
    assert np.allclose(out[3:14], (a[0, 3:14] + a[1, 3:14]) / 2, atol=1e-5)
    assert abs(z - 3.8 / 4 * (100 / 99.9)) < 1e-6
    q, out, z = T.at(0, 7.5, 6.5)
    assert np.allclose(q, (1 / 3, 1 / 3, 1 / 3), atol=1e-6)
    assert np.allclose(out[3:14], a[:, 3:14].mean(0), atol=1e-5)
    assert abs(z - 5.7 / 6 * (100 / 99.9)) < 1e-6
    # the centroid is inside: the truth is certain there, its interval holds the hand value and the restatement's
    w = T.winners()
    assert w[6, 7] == 0 and w[0, 0] == RT.BACKGROUND
    planes, mat, depth, _ = R.rasterize(m, d, v)
    rep = T.check(w, planes, mat, depth)
    assert not rep.failures, rep.failures
    assert np.allclose(planes[3:14, 6, 7], a[:, 3:14].mean(0), atol=1e-5) and abs(depth[6, 7] - 0.950951) < 1e-6


# -- power -----------------------------------------------------------------------------------------------------------

def _vs_variant(monkeypatch, change):
    orig = R.vertex_stage

    def wrong(vertices, draw, view):
        vs = orig(vertices, draw, view)
        change(vs, view)
        return vs
    monkeypatch.setattr(R, "vertex_stage", wrong)


def no_perspective(monkeypatch, defect):
    """Attributes with l_i in place of q_i: with rw = 1 step 8 gives q_i = l_i / ((l0 + l1) + l2), l_i to a rounding."""
    def change(vs, view):
        if defect:
            vs["rw"] = np.ones_like(vs["rw"])
    _vs_variant(monkeypatch, change)


def rw_is_w(monkeypatch, defect):
    def change(vs, view):
        if defect:
            with np.errstate(all="ignore"):
                vs["rw"] = (F(1.0) / vs["rw"]).astype(F)
    _vs_variant(monkeypatch, change)


def y_not_flipped(monkeypatch, defect):
    def change(vs, view):
        if defect:
            vs["Y"] = np.int64(256 * int(view.height)) - vs["Y"]
    _vs_variant(monkeypatch, change)


def sample_point_moved(monkeypatch, defect):
    """The sample point 2/256 px to the right of the pixel centre."""
    def edge_values(edges, x, y):
        px = np.int64(256) * x + np.int64(128 + (2 if defect else 0))
        py = np.int64(256) * y + np.int64(128)
        return [np.int64(dx) * (py - np.int64(ya)) - np.int64(dy) * (px - np.int64(xa)) for dx, dy, xa, ya, _ in edges]
    monkeypatch.setattr(R, "_edge_values", edge_values)


def crossing_t_reversed(monkeypatch, defect):
    """Clip crossings with t replaced by 1 - t, in the position and in the attributes."""
    class Wrong(CR._PieceVertex):
        def __init__(self, vs, ph, view, a, b=None):
            super().__init__(vs, ph, view, a, b)
            if b is not None and defect:
                with np.errstate(all="ignore"):
                    pa, pb = ph[:, a], ph[:, b]
                    self.t = t = F(1.0) - self.t
                    x, y, w = pa[0] + t * (pb[0] - pa[0]), pa[1] + t * (pb[1] - pa[1]), pa[3] + t * (pb[3] - pa[3])
                self.X, self.Y, self.z, self.rw, self.near, self.guard = CR.viewport(x, y, F(0.0), w, view)
    monkeypatch.setattr(CR, "_PieceVertex", Wrong)


def attributes_not_exchanged(m, d, v, exchange):
    """The restatement's image with step 8 redone, from its own helpers, for every triangle that setup turned over
    (A < 0 under cull none): coverage, z and q from the exchanged order, the attributes from the exchanged order too
    (``exchange``: the rules) or from the submitted order (the defect). One triangle per draw, a material per draw."""
    planes, mat, depth, stats = R.rasterize(m, d, v)
    planes = planes.copy()
    for dr in d:
        vs = R.vertex_stage(m[dr.mesh].vertices, dr, v)
        count = m[dr.mesh].indices.size - dr.first_index if dr.index_count is None else dr.index_count
        assert count == 3
        i = [int(k) for k in m[dr.mesh].indices[dr.first_index:dr.first_index + 3]]
        X, Y = [int(vs["X"][k]) for k in i], [int(vs["Y"][k]) for k in i]
        A = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
        if A >= 0:
            continue
        g = [i[0], i[2], i[1]]
        src = g if exchange else i
        y, x = np.nonzero(mat == dr.material)
        E = R._edge_values(R._edges([int(vs["X"][k]) for k in g], [int(vs["Y"][k]) for k in g]), x, y)
        l = R._barycentrics(E, -A)
        p = [l[k] * vs["rw"][g[k]] for k in range(3)]
        s = (p[0] + p[1]) + p[2]
        q = [p[k] / s for k in range(3)]
        for k in range(14):
            a = vs["a"][k]
            planes[k][y, x] = (q[0] * a[src[0]] + q[1] * a[src[1]]) + q[2] * a[src[2]]
    return planes, mat, depth, stats


def caught_share(T, image, only_back=False):
    """The share of the truth's checked geometry pixels at which the image fails the bound or names another winner."""
    w = T.winners()
    rep = T.check(w, *image[:3])
    pixels = rep.geometry
    if only_back:
        front = np.array([tr is not None and bool(tr["front"]) for tr in T.tri] + [True])
        pixels = pixels & ~front[np.where(w >= 0, w, -1)]
    assert pixels.sum() > 50
    return float((rep.bad & pixels).sum()) / float(pixels.sum()), rep


POWER_SCENES = (("plain", "one_triangle", "70x37"), ("soup", "1", "71x37"))


@pytest.mark.parametrize("defect", [True, False])
@pytest.mark.parametrize("variant", [no_perspective, rw_is_w, y_not_flipped, sample_point_moved])
@pytest.mark.parametrize("scene", POWER_SCENES, ids=lambda s: s[1])
def test_wrong_restatement_is_caught(monkeypatch, variant, scene, defect):
    """A defect in the restatement fails at >= 90% of the checked pixels of one_triangle and of a soup; the same patch
    with the defect taken out passes everywhere."""
    m, d, v = RT.scene(*scene)[:3]
    variant(monkeypatch, defect)
    share, rep = caught_share(RT.truth(*scene), R.rasterize(m, d, v))
    print(variant.__name__, scene[1], "defect" if defect else "sound", f"caught at {100 * share:.1f}% of the checked pixels")
    if defect:
        assert share >= 0.9
    else:
        assert share == 0.0 and not rep.failures, rep.failures


@pytest.mark.parametrize("exchange", [False, True])
@pytest.mark.parametrize("scene", ("one_triangle_turned", "soup"))
def test_unexchanged_attributes_are_caught(scene, exchange):
    """Vertices 1 and 2 exchanged for coverage but not for the attributes: only a triangle that setup turns over can
    show it, so one_triangle is submitted with vertices 1 and 2 the other way round under cull none, and on the soup
    the share is taken over the pixels whose winner the truth calls back facing."""
    if scene == "soup":
        m, d, v = RT.scene("soup", "1", "71x37")[:3]
        T = RT.truth("soup", "1", "71x37")
    else:
        m, d, v = C.case("one_triangle", 70, 37)
        m = [C.Mesh(m[0].vertices, np.array([0, 2, 1], np.uint32))]
        d = [C.Draw(mesh=0, material=3, cull=1)]
        T = RT.Truth(m, d, v)
    image = attributes_not_exchanged(m, d, v, exchange)
    share, rep = caught_share(T, image, only_back=True)
    print(scene, "exchanged" if exchange else "not exchanged", f"caught at {100 * share:.1f}% of the back-facing pixels")
    if exchange:
        want = R.rasterize(m, d, v)[0]
        assert np.array_equal(image[0].view(np.uint32), want.view(np.uint32))  # the helper redoes step 8 bit for bit
        assert share == 0.0 and not rep.failures, rep.failures
    else:
        assert share >= 0.9


@pytest.mark.parametrize("defect", [True, False])
@pytest.mark.parametrize("name", ["single_n1_rot0_cull1_front", "single_n2_rot0_cull1_front"])
def test_reversed_crossing_parameter_is_caught(monkeypatch, name, defect):
    """t replaced by 1 - t needs a clipped triangle: the two base triangles of the clip cases, one and two vertices
    inside."""
    m, d, v = RT.scene("clip", name, "70x37")[:3]
    crossing_t_reversed(monkeypatch, defect)
    share, rep = caught_share(RT.truth("clip", name, "70x37"), CR.rasterize(m, d, v))
    print(name, "defect" if defect else "sound", f"caught at {100 * share:.1f}% of the checked pixels")
    if defect:
        assert share >= 0.9
    else:
        assert share == 0.0 and not rep.failures, rep.failures
