"""The layer restatement (tests/raster_layer_reference.py) against the pass it takes apart:
the k-th layer's winners are, at every pixel, the k-th fragment the sequential depth-tested pass accepts
(raster_layer_reference.emulate: triangles in order over a depth buffer, accept iff z < d), the layers end after the
longest chain, and the depth plane ends as the emulation's depth buffer. No GPU: the device is held to the restatement
by tests/test_gpu_raster_layer.py."""
import numpy as np
import pytest

import raster_alpha_reference as AR
import raster_layer_cases as LC
import raster_layer_reference as LR
import raster_reference as R
from oracle import oracle as O

F = np.float32
W, H = LC.FRAMES["70x37"]

_cache = {}


def depth0(sc):
    """The opaque layer's depth (1 where it draws nothing)."""
    return AR.rasterize(sc.meshes, sc.opaque, sc.view, [], [], sc.clip_near, alpha_test=False)[2]


def peeled(name):
    if name not in _cache:
        sc = LC.case(name, W, H)
        d0 = depth0(sc)
        _cache[name] = (sc, d0, LR.peel(sc.meshes, sc.draws, sc.view, d0, sc.clip_near),
                        LR.emulate(sc.meshes, sc.draws, sc.view, d0, sc.clip_near))
    return _cache[name]


@pytest.mark.parametrize("name", LC.CASES)
def test_layers_are_the_accepted_fragments_in_order(name):
    sc, d0, layers, (prims, zs, final) = peeled(name)
    chain = len(prims)
    print(name, "chain", chain, [l.layer["layer_fragments"] for l in layers])
    if LC.CHAINS[name] is not None:
        assert chain == LC.CHAINS[name]
    assert chain >= 1
    # the layer count equals the longest chain: `chain` layers with fragments, then the empty one
    assert len(layers) == chain + 1 and layers[-1].layer["layer_fragments"] == 0
    d_prev = d0
    for k in range(chain):
        l = layers[k]
        won = l.material != R.NONE
        assert np.array_equal(won, prims[k] >= 0), k
        assert np.array_equal(l.prim[won].astype(np.int64), prims[k][won] + 1), k
        assert O.bit_equal(l.depth[won], zs[k][won]).all(), k
        # strictly nearer than what came in; a pixel without a winner passes depth_in through, floor 0xFFFFFFFF
        assert (l.depth[won] < d_prev[won]).all()
        assert O.bit_equal(l.depth[~won], d_prev[~won]).all() and (l.prim[~won] == LR.NO_FLOOR).all()
        assert l.layer["layer_fragments"] >= int(won.sum()) > 0
        d_prev = l.depth
    # the empty layer changes nothing, and the depth is the depth buffer after the pass
    last = layers[-1]
    assert (last.material == R.NONE).all() and (last.prim == LR.NO_FLOOR).all()
    assert O.bit_equal(last.depth, final).all() and O.bit_equal(d_prev, final).all()
    # the counters that do not depend on the layer are the unflagged call's
    plain = AR.rasterize(sc.meshes, sc.draws, sc.view, [], [], sc.clip_near, alpha_test=False)
    for l in layers:
        assert l.stats == plain[3] and l.clip == plain[4]


def test_first_layer_over_empty_depth_wins_by_order_not_by_depth():
    """nested_far_near: the first layer is the first-submitted (farthest) quad wherever it covers, although nearer
    fragments exist there; the unflagged call shows the nearest."""
    sc, d0, layers, _ = peeled("nested_far_near")
    plain = AR.rasterize(sc.meshes, sc.draws, sc.view, [], [], alpha_test=False)
    assert (d0 == F(1)).all()
    assert set(np.unique(layers[0].material).tolist()) == {0, R.NONE}
    assert set(np.unique(plain[1]).tolist()) == {0, 1, 2, R.NONE}
    assert [set(np.unique(l.material).tolist()) - {R.NONE} for l in layers] == [{0}, {1}, {2}, set()]
    # the last non-empty layer's depth is the nearest depth: the unflagged call's
    assert O.bit_equal(layers[-1].depth, plain[2]).all()


def test_equal_z_is_not_accepted_twice():
    sc, d0, layers, (prims, zs, final) = peeled("equal_z")
    assert len(layers) == 2
    won = layers[0].material != R.NONE
    assert (layers[0].depth[won].view(np.uint32) == 0).all()  # z = +0 everywhere
    # the second and third quads lie inside the first: every one of their fragments ties and is dropped
    assert set(np.unique(layers[0].material).tolist()) == {0, R.NONE}
    # over the cleared depth every fragment of the three quads is eligible in layer 0; in layer 1 none is
    assert layers[0].layer["layer_fragments"] == layers[0].stats["fragments"] > int(won.sum())
    assert layers[1].stats["fragments"] == layers[0].stats["fragments"] and layers[1].layer["layer_fragments"] == 0


def test_opaque_depth_hides_what_is_behind_it():
    sc, d0, layers, _ = peeled("panes_opaque")
    bg, _, over_bg, _ = peeled("panes_background")[0:4]
    assert (d0 < F(1)).any() and (d0 == F(1)).any()
    hidden = d0 < F(1)
    far = layers[0].material == 0
    assert far.any() and not (far & hidden).any()  # the w = 3 pane never shows where the opaque quad (w = 2) is
    assert (layers[0].material[hidden] != 0).all()
    assert len(layers) == 4 and len(over_bg) == 4


@pytest.mark.parametrize("bad", [np.nan, 0.0, -1.0])
def test_depth_in_nan_or_zero_gives_no_fragment(bad):
    sc = LC.case("nested_far_near", W, H)
    d = np.full((H, W), bad, F)
    l = LR.rasterize_layer(sc.meshes, sc.draws, sc.view, d)
    assert l.layer["layer_fragments"] == 0 and l.stats["fragments"] > 0
    assert (l.material == R.NONE).all() and (l.prim == LR.NO_FLOOR).all()
    assert O.bit_equal(l.depth, d).all()  # passed through, a NaN's bits included


def test_floor_of_a_finished_pixel_admits_nothing():
    """prim_in = 0xFFFFFFFF everywhere: no ordinal reaches it, whatever the depth."""
    sc = LC.case("nested_far_near", W, H)
    l = LR.rasterize_layer(sc.meshes, sc.draws, sc.view, np.ones((H, W), F), np.full((H, W), LR.NO_FLOOR, np.uint32))
    assert l.layer["layer_fragments"] == 0 and (l.material == R.NONE).all()
    zero = LR.rasterize_layer(sc.meshes, sc.draws, sc.view, np.ones((H, W), F), np.zeros((H, W), np.uint32))
    none = LR.rasterize_layer(sc.meshes, sc.draws, sc.view, np.ones((H, W), F), None)
    assert O.bit_equal(zero.planes, none.planes).all() and np.array_equal(zero.prim, none.prim)


@pytest.mark.parametrize("name", ["intersecting", "clipped_pane"])
def test_a_band_equals_the_same_rows_of_the_full_frame(name):
    sc, d0, layers, _ = peeled(name)
    for r0, r1 in ((0, 5), (5, 6), (6, H - 9), (H - 9, H)):
        depth, prim = d0[r0:r1], None
        for k, full in enumerate(layers):
            b = LR.rasterize_layer(sc.meshes, sc.draws, sc.view.rows(r0, r1), depth, prim, sc.clip_near)
            assert O.bit_equal(b.planes, full.planes[:, r0:r1]).all(), (r0, r1, k)
            assert np.array_equal(b.material, full.material[r0:r1]) and np.array_equal(b.prim, full.prim[r0:r1])
            assert O.bit_equal(b.depth, full.depth[r0:r1]).all()
            depth, prim = b.depth, b.prim


def test_clipped_pane_is_clipped_and_pieces_share_an_ordinal():
    sc, d0, layers, (prims, zs, final) = peeled("clipped_pane")
    assert sc.clip_near and layers[0].clip["clipped_near"] > 0
    assert layers[0].clip["clip_pieces"] > layers[0].clip["clipped_near"]  # some triangle has two pieces
    assert (d0 < F(1)).any()
