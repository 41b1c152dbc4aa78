"""The rasteriser's list, box and draw-table code at scale on the GPU (csrc/raster.h; DESIGN.md §12, "Kernels"): the
scenes of tests/raster_scale_cases.py -- a large list of 1,300 entries against the large kernel's 1,024 striding
workgroups in all six instantiations, the two-slot list of a clipping call with second pieces, triangle counts around
the setup kernel's workgroup, boxes of exactly 64 and 65 pixels, a box of 51 blocks off the block grid, a table of 300
draws with empty ones, coordinates next to the guard band. Every comparison is bit for bit (oracle.bit_equal, NaN
patterns equal) against the restatements of tests/raster_reference.py, raster_clip_reference.py,
raster_alpha_reference.py and raster_layer_reference.py -- all 14 planes, material, depth, the floor plane of a layer --
and every counter set exactly, in both row strides. tests/test_frontend_shapes_host.py shows that each scene reaches
the code it is named for."""
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_shape_cases as FS
import raster_alpha_cases as AC
import raster_alpha_reference as AR
import raster_cases as C
import raster_clip_reference as CR
import raster_layer_cases as LC
import raster_layer_reference as LR
import raster_reference as R
import raster_scale_cases as SC
import test_gpu_raster_alpha as TA
import test_gpu_raster_layer as TL
from conftest import ROOT
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd.renderer import ShadingContext

pytestmark = pytest.mark.gpu

ZERO_ALPHA = dict.fromkeys(AR.ALPHA_STAT_NAMES, 0)


@pytest.fixture(scope="module")
def ctx(gpu):
    c = ShadingContext(0)
    yield c
    c.close()


def run(ctx, scene, mats=(), texs=(), clip_near=False, alpha_test=False, bands=(), what=""):
    """One scene through pbr_rasterize_flags in both strides against raster_alpha_reference.rasterize (which is the two
    older restatements without their flags), all three counter sets; then the bands against the full frame's rows and
    the restatement's counters for the band."""
    m, d, v = scene
    mats, texs = list(mats), list(texs)
    want = AR.rasterize(m, d, v, mats, texs, clip_near, alpha_test=alpha_test)
    print(what, want[3], want[4], want[5])
    if not alpha_test:  # the unflagged and the clipping restatement themselves say the same
        older = CR.rasterize(m, d, v) if clip_near else R.rasterize(m, d, v) + (want[4],)
        assert O.bit_equal(older[0], want[0]).all() and np.array_equal(older[1], want[1]), what
        assert O.bit_equal(older[2], want[2]).all() and older[3:] == want[3:5], what
    for stride in FS.strides(v.width):
        got = AC.device_rasterize(ctx, m, d, v, mats, texs, clip_near, alpha_test, stride=stride)
        TA.check(got, want, v.width, f"{what} stride {stride}")
    for r0, r1 in bands:
        got = AC.device_rasterize(ctx, m, d, v, mats, texs, clip_near, alpha_test, rows=(r0, r1))
        TA.check(got, want, v.width, f"{what} rows {r0}:{r1}", rows=(r0, r1))
        band = AR.rasterize(m, d, v.rows(r0, r1), mats, texs, clip_near, alpha_test=alpha_test)
        assert got[3:] == band[3:], (what, r0, r1)
    return want


# ---- many_large: the large list past the striding workgroups, in the six large-kernel instantiations --------------

@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("alpha", [False, True], ids=["untested", "alpha"])
def test_many_large_through_rasterize_flags(ctx, clip, alpha):
    """raster_large_kernel<CLIP, ALPHA, false>: 1,300 entries (1,387 with second pieces when clipping) over 1,024
    workgroups in x: the second trip of the list loop. The unflagged scene also goes through pbr_rasterize itself and
    equals tests/raster_reference.py."""
    scene = SC.many_large(clip=clip)
    mats, texs = SC.checker_table() if alpha else ([], [])
    want = run(ctx, scene, mats, texs, clip, alpha, what=f"many_large clip {clip} alpha {alpha}")
    assert want[3]["triangles"] == SC.N_SLIVERS and want[3]["fragments"] > 100000
    if clip:
        assert want[4]["clip_pieces"] == 2 * (SC.N_SLIVERS // 10)
    if alpha:
        assert 0 < want[5]["alpha_discarded"] < want[5]["alpha_tested"] == want[3]["fragments"]
    if not clip and not alpha:
        plain = R.rasterize(*scene)
        for stride in FS.strides(scene[2].width):
            TA.check(C.device_rasterize(ctx, *scene, stride=stride) + (want[4], ZERO_ALPHA), plain + (want[4], ZERO_ALPHA),
                     scene[2].width, f"many_large pbr_rasterize stride {stride}")


@pytest.mark.parametrize("n_tris", [SC.LARGE_GRID_X, SC.LARGE_GRID_X + 1])
def test_many_large_cut_at_the_grid_boundary(ctx, n_tris):
    """gridDim.x = min(n_tris, 1024): exactly 1,024 listed triangles (one each, no second trip) and 1,025."""
    m, d, v = SC.many_large()
    run(ctx, (m, SC.cut_to(d, n_tris), v), what=f"many_large cut to {n_tris}")


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_many_large_first_three_layers(ctx, clip):
    """raster_large_kernel<CLIP, false, true> through pbr_rasterize_layer: the first three layers of the peel over an
    empty opaque layer (depth 1 everywhere), separate planes in the odd stride, aliased planes in the even one."""
    m, d, v = SC.many_large(clip=clip)
    sc = LC.Scene(m, [], d, v, clip)
    W, H = v.width, v.height
    d0 = np.ones((H, W), np.float32)
    layers, depth, prim = [], d0, None
    for _ in range(3):
        layers.append(LR.rasterize_layer(m, d, v, depth, prim, clip))
        depth, prim = layers[-1].depth, layers[-1].prim
    print("many_large layers", [l.layer["layer_fragments"] for l in layers])
    assert all(l.layer["layer_fragments"] > 10000 for l in layers)
    ctx.set_meshes(m)
    for stride, alias in zip(FS.strides(W), (False, True)):
        depth = LC.padded(d0, stride, C.SENTINEL)
        prim = LC.padded(np.zeros((H, W), np.uint32), stride, 0) if alias else None
        for k, want in enumerate(layers):
            got, counters = LC.device_layer(ctx, sc, depth, prim, stride=stride, alias=alias)
            TL.check(LC.to_host(got), counters, want, W, f"many_large clip {clip} stride {stride} layer {k}",
                     pad_prim=0 if alias else C.SENTINEL_ID)
            depth, prim = got[2], got[3]


# ---- setup workgroup edge, box threshold, block walk ----------------------------------------------------------------

@pytest.mark.parametrize("n_tris", [255, 256, 257])
def test_triangle_counts_around_the_setup_workgroup(ctx, n_tris):
    run(ctx, SC.tri_counts(n_tris), what=f"tri_counts {n_tris}")


def test_boxes_of_64_and_65_pixels_and_bands_that_make_large_small(ctx):
    """kSmallPixels: boxes of exactly 64 pixels (8x8, 64x1, 16x4, 2x32, and one cut to 8x8 by the frame's right edge)
    are rasterised by their setup lane, boxes of 65 and 66 go to the list; in the bands three listed triangles are
    small. Every band's rows equal the full frame's. Also under the other two setup kernels that take no material."""
    run(ctx, SC.box_threshold(), bands=SC.BOX_BANDS, what="box_threshold")
    run(ctx, SC.box_threshold(), clip_near=True, bands=SC.BOX_BANDS[1:3], what="box_threshold clip")


def test_a_box_of_51_blocks_whose_origin_is_off_the_block_grid(ctx):
    """blk % nbx and blk / nbx with nbx = 3 from a box at (3, 5), 51 blocks over 32 slabs: the second trip of the block
    loop; full frame and two bands (in which the box starts on the band's first row)."""
    want = run(ctx, SC.offset_blocks(), bands=SC.OFFSET_BANDS, what="offset_blocks")
    assert want[3]["fragments"] > 4000


# ---- the draw table --------------------------------------------------------------------------------------------------

def test_300_draws_with_empty_ones(ctx):
    """find_draw over a triangle prefix with ties (empty draws first, last and in runs) in the setup, large and resolve
    kernels, and over the record prefix of 300 draws in the vertex kernel; with and without near clipping."""
    want = run(ctx, SC.many_draws(), bands=FS.UNEVEN_BANDS[1:3], what="many_draws")
    assert want[3]["triangles"] == 199
    run(ctx, SC.many_draws(), clip_near=True, what="many_draws clip")


def test_every_draw_empty_is_the_background(ctx):
    """Zero triangles from 300 draws: only the vertex and resolve kernels run; the frame is the background of step 9,
    as with no draw at all, and every counter is 0."""
    m, d, v = SC.many_draws(all_empty=True)
    want = run(ctx, (m, d, v), what="many_draws all empty")
    assert want[3] == dict.fromkeys(R.STAT_NAMES, 0) and (want[1] == R.NONE).all()
    none = AC.device_rasterize(ctx, m, [], v, [], [], alpha_test=False)
    TA.check(none, want, v.width, "no draws")


# ---- magnitudes next to the guard band -------------------------------------------------------------------------------

@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_coordinates_next_to_the_guard_band(ctx, clip):
    """Vertices 20,000 to 32,767.9 pixels out: edge functions and areas up to about 2^48 through the int64 -> float
    conversions of step 6; one vertex beyond the band for contrast."""
    want = run(ctx, SC.guard_scale(clip=clip), clip_near=clip, bands=FS.UNEVEN_BANDS[:2],
               what=f"guard_scale clip {clip}")
    assert want[3]["skipped_guard_band"] >= 1 and want[3]["fragments"] > 0


# ---- the bounds-checked build ----------------------------------------------------------------------------------------

def test_bounds_checked_build_is_clean_and_equal(tmp_path, gpu):
    """raster_scale_cases.bounds_runs() -- many_large unflagged and with clipping and the alpha test, many_draws --
    under _lib/debug_bounds/libpbrshade.so in a fresh child process (PBR_LIB_PATH): no index class is flagged and the
    results equal the restatement."""
    import bounds_cases

    if not os.path.exists(C.DEBUG_LIB):
        pytest.fail(f"{C.DEBUG_LIB} missing: run `make -C physically_based_renderer_amd/csrc debug-bounds` first")
    problems = bounds_cases.debug_library_problems(bounds_cases.library_build_info(C.DEBUG_LIB), N.kernel_sources_sha())
    assert not problems, f"{C.DEBUG_LIB} is not the bounds-checked build of this checkout: " + "; ".join(problems)
    out = tmp_path / "raster_scale_dbg.npz"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "raster_scale_cases.py"), str(out)],
                       env={**os.environ, "PBR_LIB_PATH": C.DEBUG_LIB}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)  # numeric and unicode arrays only: allow_pickle stays False
    assert str(z["flavor"]) == "debug_bounds" and str(z["sources_sha"]) == N.kernel_sources_sha()
    assert (z["bounds"] < 0).all(), f"bounds violations (gbuffer/output/coverage/texel/light/lds/raster/mesh): {z['bounds']}"
    for name, m, d, v, mats, texs, clip_near, alpha_test in SC.bounds_runs():
        want = AR.rasterize(m, d, v, mats, texs, clip_near, alpha_test=alpha_test)
        c = z[name + "__stats"].tolist()
        counters = (dict(zip(sorted(want[3]), c[:6])), dict(zip(sorted(want[4]), c[6:8])), dict(zip(sorted(want[5]), c[8:])))
        TA.check((z[name + "__planes"], z[name + "__ids"], z[name + "__depth"]) + counters, want, v.width,
                 "debug-bounds " + name)
