"""pbr_rasterize on the GPU (csrc/raster.h): VS and the rasteriser from indexed meshes to the attribute
planes pbr_resolve_materials consumes. Every comparison is bit for bit (oracle.bit_equal, NaN patterns equal) against
the numpy restatement of tests/raster_reference.py -- all 14 planes, the material plane, the depth plane -- and the
statistics counters exactly. tests/test_raster_host.py checks the restatement against the rules themselves."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_cases as C
import raster_reference as R
import resolve_reference as RR
from conftest import ROOT, oracle_pass_from_constants
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import envmap
from physically_based_renderer_amd import scenes as S
from physically_based_renderer_amd.renderer import Draw, Mesh, ShadingContext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    c = ShadingContext(0)
    yield c
    c.close()


_expected = {}


def expected(name, frame):
    """The restatement of one case, computed once and shared."""
    if (name, frame) not in _expected:
        W, H = C.FRAMES[frame]
        _expected[(name, frame)] = R.rasterize(*C.case(name, W, H))
    return _expected[(name, frame)]


def check(got, want, W, what, rows=None):
    planes, ids, depth, stats = got
    eplanes, eids, edepth, estats = want
    r0, r1 = (0, planes.shape[1]) if rows is None else rows
    for k in range(14):
        eq = O.bit_equal(planes[k][r0:r1, :W], eplanes[k][r0:r1])
        assert eq.all(), f"{what}: plane {k} differs at {np.argwhere(~eq)[:4].tolist()}"
    eq = ids[r0:r1, :W] == eids[r0:r1]
    assert eq.all(), f"{what}: material differs at {np.argwhere(~eq)[:4].tolist()}"
    eq = O.bit_equal(depth[r0:r1, :W], edepth[r0:r1])
    assert eq.all(), f"{what}: depth differs at {np.argwhere(~eq)[:4].tolist()}"
    if rows is None:
        assert stats == estats, f"{what}: stats {stats} != {estats}"
    # the padding columns of a strided canvas, and the rows outside a band, are never written
    assert (planes[:, :, W:] == C.SENTINEL).all() and (depth[:, W:] == C.SENTINEL).all()
    assert (ids[:, W:] == C.SENTINEL_ID).all()
    outside = np.ones(planes.shape[1], bool)
    outside[r0:r1] = False
    assert (planes[:, outside] == C.SENTINEL).all() and (depth[outside] == C.SENTINEL).all()
    assert (ids[outside] == C.SENTINEL_ID).all()


@pytest.mark.parametrize("frame", list(C.FRAMES))
@pytest.mark.parametrize("name", C.CASES)
def test_case_equals_the_restatement(ctx, name, frame):
    """Every case of raster_cases.CASES in both frames, into an odd row stride (width + 1: the scalar stores) and into
    an even one (width: the paired stores)."""
    W, H = C.FRAMES[frame]
    m, d, v = C.case(name, W, H)
    want = expected(name, frame)
    print(name, frame, want[3])
    for stride in (W + 1, W):
        got = C.device_rasterize(ctx, m, d, v, stride=stride)
        check(got, want, W, f"{name} {frame} stride {stride}")


@pytest.mark.parametrize("name,frame", [("uv_sphere", "256x64"), ("offscreen", "70x37"), ("random_subpixel", "70x37")])
def test_row_bands_equal_the_full_frame(ctx, name, frame):
    """Uneven bands through offset pointers equal the same rows of the full frame; other rows keep the sentinel."""
    W, H = C.FRAMES[frame]
    m, d, v = C.case(name, W, H)
    want = expected(name, frame)
    for r0, r1 in ((0, 5), (5, 6), (6, H - 9), (H - 9, H)):
        got = C.device_rasterize(ctx, m, d, v, rows=(r0, r1))
        check(got, want, W, f"{name} {frame} rows {r0}:{r1}", rows=(r0, r1))
        band_stats = R.rasterize(m, d, v.rows(r0, r1))[3]
        assert got[3] == band_stats, (r0, r1)


def test_two_streams_and_a_mesh_swap(gpu):
    """Rasterisations queued alternately on two streams (each has its own scratch), the mesh set replaced while they
    are queued, more rasterisations: every result is that of the set current when it was queued. Not a shading pass:
    the statistics and kernel name of the shade before are unchanged."""
    W, H = C.FRAMES["256x64"]
    m1, d1, v1 = C.case("uv_sphere", W, H)
    m2, d2, v2 = C.case("interpenetrating", W, H)
    want1, want2 = expected("uv_sphere", "256x64"), expected("interpenetrating", "256x64")
    cfg = S.CONFIGS[2].with_size(128, 16)
    with ShadingContext(0) as ctx:
        ctx.set_pass(S.scene_pass(cfg))
        ctx.shade(S.build_gbuffer(cfg, gpu))
        stats, kernel = ctx.pass_stats(), ctx.last_kernel()
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        torch.cuda.synchronize()
        ctx.set_meshes(m1)
        outs = []
        for k in range(6):
            outs.append((want1, ctx.rasterize(d1, v1, stream=(s1, s2)[k % 2])))
        ctx.set_meshes(m2, stream=s1)  # the first set is released after the queued rasterisations
        for k in range(6):
            outs.append((want2, ctx.rasterize(d2, v2, stream=(s2, s1)[k % 2])))
        assert ctx.pass_stats() == stats and ctx.last_kernel() == kernel
        assert ctx.raster_stats(s1) == want2[3] and ctx.raster_stats(s2) == want2[3]
        torch.cuda.synchronize()
        for k, (want, at) in enumerate(outs):
            got = (at.planes.cpu().numpy(), at.material.cpu().numpy().view(np.uint16), at.depth.cpu().numpy())
            assert O.bit_equal(got[0], want[0]).all(), k
            assert np.array_equal(got[1], want[1]) and O.bit_equal(got[2], want[2]).all(), k


def test_argument_errors(gpu):
    W, H = 32, 16
    m, d, v = C.case("one_triangle", W, H)
    inv = N.PBR_ERR_INVALID_ARGUMENT
    lib = N.lib()
    with ShadingContext(0) as ctx:
        with pytest.raises(N.PbrError) as e:  # before pbr_set_meshes
            ctx.rasterize([Draw(mesh=0, index_count=3)], v)
        assert e.value.status == N.PBR_ERR_NOT_READY
        assert ctx.raster_stats() == dict.fromkeys(R.STAT_NAMES, 0)
        bad = Mesh(m[0].vertices, np.array([0, 1, 3], np.uint32))  # an index == n_vertices
        with pytest.raises(N.PbrError) as e:
            ctx.set_meshes([bad])
        assert e.value.status == inv
        desc = (N.MeshDesc * 1)()
        desc[0].n_vertices, desc[0].n_indices = 3, 3  # null vertex and index pointers
        assert lib.pbr_set_meshes(ctx.handle, desc, 1, None) == inv
        assert lib.pbr_set_meshes(ctx.handle, None, 1, None) == inv
        assert lib.pbr_set_meshes(ctx.handle, desc, -1, None) == inv
        ctx.set_meshes(m)
        for bad_draw in (Draw(mesh=1, index_count=3), Draw(mesh=-1, index_count=3), Draw(index_count=4),
                         Draw(first_index=1, index_count=3), Draw(first_index=-3, index_count=3),
                         Draw(index_count=-3), Draw(index_count=3, cull=2)):
            with pytest.raises(N.PbrError) as e:
                ctx.rasterize([bad_draw], v)
            assert e.value.status == inv, bad_draw
        at = ctx.rasterize(d, v)
        c_view, t = v.to_c(), N.RasterTargets()
        c_draw = (N.DrawDesc * 1)(d[0].to_c(m))
        assert lib.pbr_rasterize(ctx.handle, c_draw, 1, ctypes.byref(c_view), ctypes.byref(t), None) == inv  # NULL planes
        assert lib.pbr_rasterize(ctx.handle, None, 1, ctypes.byref(c_view), ctypes.byref(t), None) == inv
        for rows in ((3, 2), (-1, 4), (0, H + 1)):
            with pytest.raises(N.PbrError) as e:
                ctx.rasterize(d, v.rows(*rows))
            assert e.value.status == inv, rows
        # more than 2^32 - 2 triangles in one call: 4097 draws of 2^20 triangles
        big = Mesh(m[0].vertices, np.tile(np.array([0, 1, 2], np.uint32), 1 << 20))
        ctx.set_meshes([big])
        with pytest.raises(N.PbrError) as e:
            ctx.rasterize([Draw()] * 4097, v)
        assert e.value.status == inv
        ctx.set_meshes(m)  # the failed calls left the context usable
        again = ctx.rasterize(d, v)
        torch.cuda.synchronize()
        assert O.bit_equal(again.planes.cpu().numpy(), at.planes.cpu().numpy()).all()
        assert ctx.raster_stats()["triangles"] == 1


def test_bounds_checked_build_is_clean_and_equal(tmp_path, gpu):
    """raster_cases.BOUNDS_CASES under _lib/debug_bounds/libpbrshade.so in a fresh child process (PBR_LIB_PATH), which
    first checks which library it loaded: the results equal the restatement and no index class -- mesh data, draw
    table, vertex records, large list, visibility words, plane stores -- is flagged."""
    import bounds_cases

    if not os.path.exists(C.DEBUG_LIB):
        pytest.fail(f"{C.DEBUG_LIB} missing: run `make -C physically_based_renderer_amd/csrc debug-bounds` first")
    problems = bounds_cases.debug_library_problems(bounds_cases.library_build_info(C.DEBUG_LIB), N.kernel_sources_sha())
    assert not problems, f"{C.DEBUG_LIB} is not the bounds-checked build of this checkout: " + "; ".join(problems)
    out = tmp_path / "raster_dbg.npz"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "raster_cases.py"), str(out)],
                       env={**os.environ, "PBR_LIB_PATH": C.DEBUG_LIB}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)  # numeric and unicode arrays only: allow_pickle stays False
    assert str(z["flavor"]) == "debug_bounds" and str(z["sources_sha"]) == N.kernel_sources_sha()
    assert (z["bounds"] < 0).all(), f"bounds violations (gbuffer/output/coverage/texel/light/lds/raster/mesh): {z['bounds']}"
    for name, frame in C.BOUNDS_CASES:
        key = f"{name}_{frame}"
        want = expected(name, frame)
        stats = dict(zip(sorted(want[3]), z[key + "__stats"].tolist()))
        check((z[key + "__planes"], z[key + "__ids"], z[key + "__depth"], stats), want, C.FRAMES[frame][0],
              "debug-bounds " + key)


@pytest.fixture(scope="module")
def reference_frame():
    """The reference scene's 58 spheres (12 x 6 facets) at 160x90 from the overview camera, restated once."""
    cfg = S.REFERENCE_SCENE.with_size(160, 90).with_camera(*S.OVERVIEW_CAMERA)
    meshes, draws = S.reference_scene_draws(12, 6)
    view = S.reference_scene_view(cfg)
    return cfg, meshes, draws, view, R.rasterize(meshes, draws, view)


def test_rasterise_resolve_shade_equals_the_oracle(gpu, reference_frame):
    """End to end: rasterize -> resolve -> shade_frame. The rasterised planes equal the restatement; the resolved
    G-buffer equals the resolve's restatement on them, for both filters; the frame (exact mode, sky pass on the
    resolved coverage) equals the oracle's on those planes bit for bit, the faithful mode within 1e-5."""
    cfg, meshes, draws, view, want = reference_frame
    planes, ids, depth, stats = want
    assert stats["triangles"] == 58 * 12 * 2 * 5 and stats["backface_culled"] > 58 * 40
    assert 0.1 < (ids != R.NONE).mean() < 0.9 and set(np.unique(ids).tolist()) >= set(range(58))
    mats, texs = S.scene_materials(cfg)
    pc = S.scene_pass(cfg)
    sky = envmap.procedural_sky_rgba16(128, 64)
    with ShadingContext(0) as ctx:
        ctx.set_meshes(meshes)
        ctx.set_materials(mats, texs)
        ctx.set_sky_map(sky)
        at = ctx.rasterize(draws, view)
        assert ctx.raster_stats() == stats
        torch.cuda.synchronize()
        assert O.bit_equal(at.planes.cpu().numpy(), planes).all()
        assert np.array_equal(at.material.cpu().numpy().view(np.uint16), ids)
        assert O.bit_equal(at.depth.cpu().numpy(), depth).all()
        for filt in (RR.LINEAR, RR.POINT):
            rwant = RR.resolve(planes, ids, mats, texs, filt)
            gb, cov = ctx.resolve(at, filt)
            torch.cuda.synchronize()
            assert O.bit_equal(gb.planes.cpu().numpy(), rwant[0]).all(), filt
            assert O.bit_equal(gb.opacity.cpu().numpy(), rwant[1]).all(), filt
            assert np.array_equal(cov.cpu().numpy(), rwant[2]) and np.array_equal(rwant[2] != 0, ids != R.NONE)
            ctx.set_pass(pc)
            frame = ctx.shade_frame(gb, coverage=cov).cpu().numpy()
            ref = O.shade_frame(list(rwant[0]), oracle_pass_from_constants(pc), pc.light_array(), None, sky, rwant[2],
                                O.OUTPUT_RGBA32F, n_threads=8)
            print(f"rasterised reference scene, filter {filt}: bit-identical {O.bit_equal(frame, ref).mean():.6f}")
            assert O.bit_equal(frame, ref).all(), filt
        pc.flags |= N.PBR_FLAG_FAITHFUL
        ctx.set_pass(pc)
        faithful = ctx.shade_frame(gb, coverage=cov).cpu().numpy()
        pc.flags &= ~N.PBR_FLAG_FAITHFUL
    err = O.rel_err(faithful, ref).max()
    print(f"faithful max_rel {err:.3g}")
    assert err <= 1e-5
