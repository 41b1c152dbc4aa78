"""Every front-end entry point on the GPU at the frames of tests/frontend_shape_cases.py: an odd width of more than one
tile (71x37), the tile's last column missing and a lone column in a second tile (63x5, 65x2), and frames of one pixel,
one column and one row (1x1, 1x9, 3x1), each in an odd row stride (the scalar accesses) and the next even one (the
paired accesses, whose last pair has only its first half inside the frame). pbr_rasterize, pbr_rasterize_flags and
pbr_rasterize_layer and pbr_resolve_materials, pbr_resolve_materials_mip and
pbr_resolve_materials_aniso (§11) are held bit for bit (oracle.bit_equal, NaN patterns equal) to the existing numpy
restatements, counters exactly. For the resolves the input padding column holds a valid-looking pixel (`pad=`), so a
kernel that took it, or the row below an odd-height band, for a quad partner gives another answer:
tests/test_frontend_shapes_host.py asserts that for every such case."""
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_shape_cases as FS
import raster_alpha_cases as AC
import raster_alpha_reference as AR
import raster_cases as C
import raster_clip_cases as CC
import raster_clip_reference as CR
import raster_layer_cases as LC
import raster_layer_reference as LR
import raster_reference as R
import resolve_aniso_cases as RAC
import resolve_aniso_reference as RA
import resolve_cases as RC
import resolve_mip_cases as MC
import resolve_mip_reference as RM
import resolve_reference as RR
import test_gpu_raster as TR
import test_gpu_raster_alpha as TA
import test_gpu_raster_clip as TC
import test_gpu_raster_layer as TL
import test_gpu_resolve_mip as TM
from conftest import ROOT
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd.renderer import ShadingContext

pytestmark = pytest.mark.gpu

RASTER_RUNS = [(FS.BIG, name) for name in C.CASES] + [(f, name) for f in FS.SMALL for name in FS.SMALL_RASTER_CASES]
FLAG_RUNS = [(f, name) for f in FS.FLAG_FRAMES for name in FS.CLIP_CASES]
ALPHA_RUNS = [(f, name) for f in FS.FLAG_FRAMES for name in FS.ALPHA_CASES]
LAYER_RUNS = [(f, name) for f in FS.FLAG_FRAMES for name in FS.LAYER_CASES]


def ids_of(runs):
    return [f"{FS.frame_id(f)}-{name}" for f, name in runs]


@pytest.fixture(scope="module")
def ctx(gpu):
    c = ShadingContext(0)
    yield c
    c.close()


# ---- the rasteriser ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame,name", RASTER_RUNS, ids=ids_of(RASTER_RUNS))
def test_rasterize_equals_the_restatement(ctx, frame, name):
    W, H = frame
    m, d, v = C.case(name, W, H)
    want = R.rasterize(m, d, v)
    print(name, frame, want[3])
    for stride in FS.strides(W):
        TR.check(C.device_rasterize(ctx, m, d, v, stride=stride), want, W, f"{name} {W}x{H} stride {stride}")


@pytest.mark.parametrize("name", ["uv_sphere", "offscreen", "random_subpixel"])
def test_rasterize_row_bands_equal_the_full_frame(ctx, name):
    """Uneven bands of the 71x37 frame through offset pointers, in the paired stride (72: every band's pointers stay
    8-byte aligned) and the scalar one."""
    W, H = FS.BIG
    m, d, v = C.case(name, W, H)
    want = R.rasterize(m, d, v)
    for r0, r1 in FS.UNEVEN_BANDS:
        for stride in FS.strides(W):
            got = C.device_rasterize(ctx, m, d, v, stride=stride, rows=(r0, r1))
            TR.check(got, want, W, f"{name} rows {r0}:{r1} stride {stride}", rows=(r0, r1))
            assert got[3] == R.rasterize(m, d, v.rows(r0, r1))[3], (r0, r1)


@pytest.mark.parametrize("frame,name", FLAG_RUNS, ids=ids_of(FLAG_RUNS))
def test_rasterize_flags_clip_near_equals_the_restatement(ctx, frame, name):
    W, H = frame
    m, d, v = CC.case(name, W, H)
    want = CR.rasterize(m, d, v)
    print(name, frame, want[3], want[4])
    for stride in FS.strides(W):
        TC.check(CC.device_rasterize(ctx, m, d, v, stride=stride), want, W, f"{name} {W}x{H} stride {stride}")


@pytest.mark.parametrize("frame,name", ALPHA_RUNS, ids=ids_of(ALPHA_RUNS))
def test_rasterize_flags_alpha_test_equals_the_restatement(ctx, frame, name):
    W, H = frame
    scene = AC.case(name, W, H)
    want = AR.rasterize(*scene)
    print(name, frame, want[3], want[4], want[5])
    for stride in FS.strides(W):
        TA.check(AC.device_rasterize(ctx, *scene, stride=stride), want, W, f"{name} {W}x{H} stride {stride}")


@pytest.mark.parametrize("frame,name", LAYER_RUNS, ids=ids_of(LAYER_RUNS))
def test_rasterize_layer_peels_to_the_restatement(ctx, frame, name):
    """Every layer until layer_fragments is 0: separate planes in the odd stride, aliased depth and floor planes in the
    even one."""
    W, H = frame
    sc = LC.case(name, W, H)
    d0 = TL.host_depth0(sc)
    layers = LR.peel(sc.meshes, sc.draws, sc.view, d0, sc.clip_near)
    print(name, frame, [l.layer["layer_fragments"] for l in layers])
    odd, even = FS.strides(W)
    TL.peel_on_device(ctx, sc, d0, layers, W, odd, False, f"{name} {W}x{H} separate")
    TL.peel_on_device(ctx, sc, d0, layers, W, even, True, f"{name} {W}x{H} aliased")


# ---- the material resolve ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rtable():
    return RC.table()


@pytest.fixture(scope="module")
def rctx(gpu, rtable):
    c = ShadingContext(0)
    c.set_materials(*rtable)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table():
    return MC.table()


@pytest.fixture(scope="module")
def chains(table):
    return [RM.build_mips(t) for t in table[1]]


@pytest.fixture(scope="module")
def mctx(gpu, table):
    c = ShadingContext(0)
    c.set_materials(*table)
    c.generate_mips()
    yield c
    c.close()


@pytest.mark.parametrize("filt", [RR.POINT, RR.LINEAR], ids=["point", "linear"])
@pytest.mark.parametrize("frame", FS.ODD_FRAMES, ids=FS.frame_id)
def test_resolve_equals_the_restatement(rctx, rtable, frame, filt):
    """resolve_cases.attributes through every material (the 71x37 frame holds every special UV under every material;
    the small ones what fits)."""
    W, H = frame
    attrs, ids = RC.attributes(H, W, len(rtable[0]), seed=W + 3 * H)
    want = RR.resolve(attrs, ids, *rtable, filt)
    for stride in FS.strides(W):
        got = RC.device_resolve(rctx, attrs, ids, filt, stride, pad=True)
        TM.check(got, want, W, f"resolve {W}x{H} filter {filt} stride {stride}")


def mip_inputs(frame, n_materials):
    """[(name, attrs, ids)]: the ramps under each of their materials, and the special UVs with valid partners."""
    W, H = frame
    cases = [(f"ramp {t} m{m}",) + FS.ramp_case(H, W, t, m) for t in FS.RAMP_TEXELS for m in FS.RAMP_MATERIALS]
    return cases + [("special",) + FS.special_case(H, W, n_materials)]


@pytest.mark.parametrize("bias", FS.BIASES)
@pytest.mark.parametrize("frame", FS.ODD_FRAMES, ids=FS.frame_id)
def test_resolve_mip_equals_the_restatement(mctx, table, chains, frame, bias):
    W, H = frame
    for name, attrs, ids in mip_inputs(frame, len(table[0])):
        want = RM.resolve_mip(attrs, ids, *table, bias, chains=chains)
        for stride in FS.strides(W):
            got = MC.device_resolve_mip(mctx, attrs, ids, bias, stride, pad=True)
            TM.check(got, want, W, f"mip {name} {W}x{H} bias {bias} stride {stride}")


@pytest.mark.parametrize("m", FS.ANISOTROPIES)
@pytest.mark.parametrize("frame", FS.ODD_FRAMES, ids=FS.frame_id)
def test_resolve_aniso_equals_the_restatement(mctx, table, chains, frame, m):
    W, H = frame
    for name, attrs, ids in mip_inputs(frame, len(table[0])):
        want = RA.resolve_aniso(attrs, ids, *table, m, 0.0, chains=chains)
        for stride in FS.strides(W):
            got = RAC.device_resolve_aniso(mctx, attrs, ids, m, 0.0, stride, pad=True)
            TM.check(got, want, W, f"aniso {name} {W}x{H} M {m} stride {stride}")


@pytest.mark.parametrize("m,bias", [(16, 0.0), (8, 0.5)])
def test_resolve_aniso_per_quad_footprints_at_71_columns(mctx, table, chains, m, bias):
    """resolve_aniso_cases' per-quad footprints, tap counts 1 .. 16 side by side, widened to 71 columns: the last
    column's quads are half outside the frame."""
    W, H = FS.BIG
    attrs, ids = FS.quads_case(H, W)
    want = RA.resolve_aniso(attrs, ids, *table, m, bias, chains=chains)
    for stride in FS.strides(W):
        got = RAC.device_resolve_aniso(mctx, attrs, ids, m, bias, stride, pad=True)
        TM.check(got, want, W, f"quads M {m} stride {stride}")


def check_band(band, want, rows, W, what):
    """A device result of a row band against a restatement of those rows; every other row keeps the sentinel."""
    r0, r1 = rows
    inside = tuple(b[..., r0:r1, :] for b in band)
    TM.check(inside, want, W, what)
    for b in band:
        outside = np.delete(b, np.s_[r0:r1], axis=-2)
        assert (outside == (RC.SENTINEL_U8 if b.dtype == np.uint8 else RC.SENTINEL)).all(), what


@pytest.mark.parametrize("call", ["mip", "aniso"])
def test_odd_height_bands_that_end_inside_the_frame(mctx, table, chains, call):
    """Rows (0, 5) and (6, 13) of the 37-row frame: the band's last row has no y partner inside the call's height, though
    the row below lies in memory behind it with the same id and a continuing ramp, so these bands equal the restatement
    of the band alone, not the frame's rows ("Bands"); rows (12, 37) end with the frame and equal it."""
    W, H = FS.BIG
    for name, (attrs, ids) in FS.band_cases(H, W).items():
        if call == "mip":
            ref = lambda a, i: RM.resolve_mip(a, i, *table, 0.25, chains=chains)  # noqa: E731
            dev = lambda stride, rows: MC.device_resolve_mip(mctx, attrs, ids, 0.25, stride, rows=rows, pad=True)  # noqa: E731
        else:
            ref = lambda a, i: RA.resolve_aniso(a, i, *table, 8, 0.25, chains=chains)  # noqa: E731
            dev = lambda stride, rows: RAC.device_resolve_aniso(mctx, attrs, ids, 8, 0.25, stride, rows=rows, pad=True)  # noqa: E731
        full = ref(attrs, ids)
        for r0, r1 in FS.INNER_BANDS:
            alone = ref(attrs[:, r0:r1], ids[r0:r1])
            assert not O.bit_equal(alone[0][:, -1], full[0][:, r1 - 1]).all()
            for stride in FS.strides(W):
                check_band(dev(stride, (r0, r1)), alone, (r0, r1), W, f"{call} {name} rows {r0}:{r1} stride {stride}")
        r0, r1 = FS.LAST_BAND
        for stride in FS.strides(W):
            check_band(dev(stride, (r0, r1)), tuple(f[..., r0:r1, :] for f in full), (r0, r1), W,
                       f"{call} {name} rows {r0}:{r1} stride {stride}")


def test_bounds_checked_build_is_clean_and_equal(tmp_path, gpu):
    """frontend_shape_cases.bounds_cases() -- a trilinear and an anisotropic resolve at 71 columns in both strides,
    valid-looking padding -- under _lib/debug_bounds/libpbrshade.so in a fresh child process (PBR_LIB_PATH): no index
    class is flagged and the results equal the restatement."""
    import bounds_cases

    if not os.path.exists(RC.DEBUG_LIB):
        pytest.fail(f"{RC.DEBUG_LIB} missing: run `make -C physically_based_renderer_amd/csrc debug-bounds` first")
    problems = bounds_cases.debug_library_problems(bounds_cases.library_build_info(RC.DEBUG_LIB), N.kernel_sources_sha())
    assert not problems, f"{RC.DEBUG_LIB} is not the bounds-checked build of this checkout: " + "; ".join(problems)
    out = tmp_path / "frontend_shapes_dbg.npz"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "frontend_shape_cases.py"), str(out)],
                       env={**os.environ, "PBR_LIB_PATH": RC.DEBUG_LIB}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)  # numeric and unicode arrays only: allow_pickle stays False
    assert str(z["flavor"]) == "debug_bounds" and str(z["sources_sha"]) == N.kernel_sources_sha()
    assert (z["bounds"] < 0).all(), f"bounds violations (gbuffer/output/coverage/texel/light/lds): {z['bounds']}"
    mats, texs, cases = FS.bounds_cases()
    for name, call, attrs, ids, m, bias, stride in cases:
        got = (z[name + "__planes"], z[name + "__opacity"], z[name + "__coverage"])
        want = (RM.resolve_mip(attrs, ids, mats, texs, bias) if call == "mip" else
                RA.resolve_aniso(attrs, ids, mats, texs, m, bias))
        TM.check(got, want, attrs.shape[2], "debug-bounds " + name)
