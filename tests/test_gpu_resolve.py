"""pbr_resolve_materials on the GPU (material_resolve.h): the first half of PS (Default.hlsl:50-116)
-- normalize(NormalW), the material texture fetches, the F0 resolve, NormalSampleToWorldSpace, the ALPHA_TEST opacity
fetch -- from interpolated attributes to a G-buffer on the device. Every comparison is bit for bit (oracle.bit_equal,
NaN patterns equal) against the numpy fp32 restatement of tests/resolve_reference.py, which tests/test_resolve_host.py
ties to the host fill."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resolve_cases as C
import resolve_reference as R
from conftest import ROOT, oracle_pass_from_constants
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import envmap
from physically_based_renderer_amd import scenes as S
from physically_based_renderer_amd.renderer import Attributes, Material, PassConstants, ShadingContext

pytestmark = pytest.mark.gpu

FILTERS = {"point": N.PBR_FILTER_POINT, "linear": N.PBR_FILTER_LINEAR}
SHAPES = {"70x3": (3, 70), "256x8": (8, 256)}


@pytest.fixture(scope="module")
def table():
    return C.table()


@pytest.fixture(scope="module")
def ctx(gpu, table):
    c = ShadingContext(0)
    c.set_materials(*table)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames(table):
    """shape name -> (attrs, ids), computed once."""
    return {k: C.attributes(h, w, len(table[0]), seed=w) for k, (h, w) in SHAPES.items()}


_expected = {}


def expected(table, key, attrs, ids, filt):
    """The restatement of one case, computed once and shared."""
    if (key, filt) not in _expected:
        _expected[(key, filt)] = R.resolve(attrs, ids, table[0], table[1], filt)
    return _expected[(key, filt)]


def check(got, want, w, what):
    (planes, opacity, cov), (eplanes, eopacity, ecov) = got, want
    for i, name in enumerate(N.PLANE_NAMES):
        eq = O.bit_equal(planes[i][:, :w], eplanes[i])
        assert eq.all(), f"{what}: plane {name} differs at {np.argwhere(~eq)[:4].tolist()}"
    eq = O.bit_equal(opacity[:, :w], eopacity)
    assert eq.all(), f"{what}: opacity differs at {np.argwhere(~eq)[:4].tolist()}"
    assert np.array_equal(cov[:, :w], ecov), f"{what}: coverage"
    # the padding columns of a strided canvas are never written
    assert (planes[:, :, w:] == C.SENTINEL).all() and (opacity[:, w:] == C.SENTINEL).all()
    assert (cov[:, w:] == C.SENTINEL_U8).all()


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("shape,stride", [("70x3", 70), ("70x3", 71), ("256x8", 256)])
def test_random_attributes_equal_the_restatement(ctx, table, frames, shape, stride, filt):
    """Every flag combination, texture size class and channel count; UVs negative, > 1, exactly 0 and 1, on texel
    edges, NaN, +-inf, 3e9; a zero-length NormalW; background ids 0xFFFF and count + 1. Stride 71 takes the scalar
    accesses, the even strides the paired ones."""
    attrs, ids = frames[shape]
    assert (ids == N.PBR_MATERIAL_NONE).any() and (ids == len(table[0]) + 1).any()
    assert set(range(len(table[0]))) <= set(ids.ravel().tolist())
    want = expected(table, shape, attrs, ids, FILTERS[filt])
    assert np.isnan(want[0][3:6]).any()  # the zero-length normal
    got = C.device_resolve(ctx, attrs, ids, FILTERS[filt], stride)
    check(got, want, attrs.shape[2], f"{shape} stride {stride} {filt}")


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("layout", ["uniform", "checker"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_uniform_and_per_lane_paths_equal_the_restatement(ctx, table, frames, shape, layout, filt):
    """The same attributes with the material plane rearranged: (a) one material per wave (64 x 2 pixels): the
    wave-uniform record path; (b) materials alternating pixel by pixel: the per-lane path."""
    attrs, _ = frames[shape]
    h, w = SHAPES[shape]
    ids = C.uniform_ids(h, w, len(table[0])) if layout == "uniform" else C.checker_ids(h, w, len(table[0]))
    want = expected(table, f"{shape}/{layout}", attrs, ids, FILTERS[filt])
    got = C.device_resolve(ctx, attrs, ids, FILTERS[filt])
    check(got, want, w, f"{shape} {layout} {filt}")


CFG4 = S.CONFIGS[4].with_size(192, 128)


@pytest.fixture(scope="module")
def cfg4_host():
    planes, _ = S.fill_gbuffer_host(CFG4)
    return planes


def test_config4_resolve_is_the_host_fill_and_shades_like_it(gpu, cfg4_host):
    """Config 4 at 192x128: the device resolve of pbr_attributes_fill's attributes equals pbr_gbuffer_fill's planes; the
    resolved G-buffer shaded under config 4's pass (exact mode) equals the oracle on the host planes bit for bit, the
    faithful mode within the project's 1e-5."""
    planes = cfg4_host
    pc = S.scene_pass(CFG4)
    assert pc.flags & N.PBR_FLAG_F0_PLANE and not pc.flags & N.PBR_FLAG_FAITHFUL
    ref = O.shade(list(planes), oracle_pass_from_constants(pc), pc.light_array(), None, n_threads=16)
    with ShadingContext(0) as ctx:
        ctx.set_materials(*S.scene_materials(CFG4))
        gb, cov = ctx.resolve(S.build_attributes(CFG4, gpu))
        torch.cuda.synchronize()
        got = gb.planes.cpu().numpy()
        for i, name in enumerate(N.PLANE_NAMES):
            assert O.bit_equal(got[i], planes[i]).all(), name
        assert (cov.cpu().numpy() == 1).all() and (gb.opacity.cpu().numpy() == 1.0).all()
        ctx.set_pass(pc)
        exact = ctx.shade(gb).cpu().numpy()
        pc.flags |= N.PBR_FLAG_FAITHFUL
        ctx.set_pass(pc)
        faithful = ctx.shade(gb).cpu().numpy()
    print(f"cfg4 192x128 resolved: exact bit-identical {O.bit_equal(exact, ref).mean():.6f} "
          f"max_rel {O.rel_err(exact, ref).max():.3g}; faithful max_rel {O.rel_err(faithful, ref).max():.3g}")
    assert O.bit_equal(exact, ref).all()
    assert O.rel_err(faithful, ref).max() <= 1e-5


@pytest.mark.parametrize("filt", list(FILTERS))
def test_row_bands_equal_the_full_frame(ctx, table, frames, filt):
    """Three uneven bands through offset pointers; rows outside a band keep the canvas's sentinel."""
    attrs, ids = frames["256x8"]
    full = C.device_resolve(ctx, attrs, ids, FILTERS[filt])
    for r0, r1 in ((0, 3), (3, 4), (4, 8)):
        band = C.device_resolve(ctx, attrs, ids, FILTERS[filt], rows=(r0, r1))
        for b, f in zip(band, full):
            inside, outside = b[..., r0:r1, :], np.delete(b, np.s_[r0:r1], axis=-2)
            if b.dtype == np.uint8:
                assert np.array_equal(inside, f[..., r0:r1, :]) and (outside == C.SENTINEL_U8).all(), (r0, r1)
            else:
                assert O.bit_equal(inside, f[..., r0:r1, :]).all() and (outside == C.SENTINEL).all(), (r0, r1)


def shading_attributes(h, w, n_materials, seed):
    """Attributes a lit pass can shade: unit-length-ish normals, finite UVs."""
    rng = np.random.default_rng(seed)
    a = np.empty((14, h, w), np.float32)
    a[0:3] = rng.uniform(-10, 10, (3, h, w))
    n = rng.normal(size=(3, h, w))
    a[3:6] = n / np.linalg.norm(n, axis=0) * rng.uniform(0.5, 2.0, (h, w))
    a[6:12] = rng.normal(size=(6, h, w))
    a[12:14] = rng.uniform(-1.0, 2.0, (2, h, w))
    return a, rng.integers(0, n_materials, (h, w)).astype(np.uint16)


def test_resolved_opacity_drives_alpha_test_shading(gpu):
    """ALPHA_TEST materials: the resolved opacity plane feeds PBR_FLAG_ALPHA_TEST; clipped pixels keep the canvas,
    the others get alpha = opacity; the frame equals the oracle on the restatement's planes."""
    rng = np.random.default_rng(11)
    texs = [rng.integers(0, 256, (64, 64), dtype=np.uint8), rng.integers(0, 256, (5, 3, 3), dtype=np.uint8),
            rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)]
    mats = [Material(diffuse_albedo=(0.7, 0.6, 0.5), metallic=0.2, roughness=0.4, flags=C.AT, tex=(-1, -1, -1, -1, -1, 0)),
            Material(flags=C.AT | C.D | C.NM, roughness=0.6, tex=(2, -1, -1, -1, 2, 1)),
            Material(diffuse_albedo=(0.2, 0.9, 0.3), roughness=0.3, opacity=0.05),   # constant opacity: clipped
            Material(diffuse_albedo=(0.9, 0.2, 0.3), roughness=0.8, opacity=0.7)]
    h, w = 8, 256
    attrs, ids = shading_attributes(h, w, len(mats), 5)
    planes, opacity, _ = R.resolve(attrs, ids, mats, texs, R.POINT)
    lights = np.zeros((3, 12), np.float32)
    lights[:, 0:3] = rng.uniform(1, 50, (3, 3))
    lights[:, 8:11] = rng.uniform(-20, 20, (3, 3))
    pc = PassConstants(eye_pos_w=(0.0, 2.0, -30.0), num_point_lights=3, lights_array=lights,
                       flags=N.PBR_FLAG_ALPHA_TEST | N.PBR_FLAG_F0_PLANE, opacity=0.5)
    ref = O.shade(list(planes) + [opacity], oracle_pass_from_constants(pc), lights)
    with ShadingContext(0) as ctx:
        ctx.set_materials(mats, texs)
        gb, _ = ctx.resolve(Attributes.from_host(attrs, ids, gpu))
        ctx.set_pass(pc)
        out = torch.full((h, w, 4), O.UNTOUCHED_F32, dtype=torch.float32, device=gpu)
        ctx.shade(gb, out)
        torch.cuda.synchronize()
        got, got_opacity = out.cpu().numpy(), gb.opacity.cpu().numpy()
    assert O.bit_equal(got_opacity, opacity).all()
    clipped = opacity - np.float32(0.1) < 0
    assert 0 < clipped.sum() < clipped.size and (ids == 2)[clipped].any() and (ids < 2)[clipped].any()
    assert (got[clipped] == O.UNTOUCHED_F32).all()
    assert O.bit_equal(got[~clipped][:, 3], opacity[~clipped]).all()
    print(f"alpha test: {int(clipped.sum())} clipped, bit-identical {O.bit_equal(got, ref).mean():.6f}")
    assert O.bit_equal(got, ref).all()


@pytest.mark.parametrize("camera", [None, S.OVERVIEW_CAMERA], ids=["default", "overview"])
def test_reference_scene_resolve_and_frame(gpu, camera):
    """The reference's 58 spheres at 160x90: the device resolve equals the restatement (both filters), and
    shade_frame with the sky pass on the resolved coverage equals the oracle's frame on the restatement's planes."""
    cfg = S.REFERENCE_SCENE.with_size(160, 90)
    if camera is not None:
        cfg = cfg.with_camera(*camera)
    attrs, ids = S.fill_attributes_host(cfg)
    mats, texs = S.scene_materials(cfg)
    pc = S.scene_pass(cfg)
    sky = envmap.procedural_sky_rgba16(128, 64)
    with ShadingContext(0) as ctx:
        ctx.set_materials(mats, texs)
        ctx.set_pass(pc)
        ctx.set_sky_map(sky)
        at = Attributes.from_host(attrs, ids, gpu)
        for filt in (R.LINEAR, R.POINT):
            want = R.resolve(attrs, ids, mats, texs, filt)
            gb, cov = ctx.resolve(at, filt)
            torch.cuda.synchronize()
            got = gb.planes.cpu().numpy()
            for i, name in enumerate(N.PLANE_NAMES):
                assert O.bit_equal(got[i], want[0][i]).all(), (filt, name)
            assert O.bit_equal(gb.opacity.cpu().numpy(), want[1]).all()
            assert np.array_equal(cov.cpu().numpy(), want[2]) and 0 < want[2].sum() < want[2].size
        frame = ctx.shade_frame(gb, coverage=cov).cpu().numpy()  # the point-filtered G-buffer
    ref = O.shade_frame(list(want[0]), oracle_pass_from_constants(pc), pc.light_array(), None, sky, want[2],
                        O.OUTPUT_RGBA32F, n_threads=8)
    print(f"reference scene frame: bit-identical {O.bit_equal(frame, ref).mean():.6f}")
    assert O.bit_equal(frame, ref).all()


def test_set_materials_twice_across_streams_and_stats_untouched(gpu, table):
    """A larger table, resolves queued on two streams, a smaller table set while they are queued, more resolves: each
    result is that of the table current when it was queued. A resolve is not a shading pass: the statistics and the
    kernel name of the shade before it are reported unchanged."""
    big_m, big_t = table
    small_m = [Material(diffuse_albedo=(0.1, 0.2, 0.3), metallic=0.9, roughness=0.1, opacity=0.4),
               Material(flags=C.R_, tex=(-1, -1, -1, 0, -1, -1))]
    small_t = [np.random.default_rng(2).integers(0, 256, (5, 3), dtype=np.uint8)]
    h, w = 128, 192
    attrs, ids = shading_attributes(h, w, len(big_m), 9)
    want_big = R.resolve(attrs, ids, big_m, big_t, R.LINEAR)
    want_small = R.resolve(attrs, ids, small_m, small_t, R.LINEAR)  # ids >= 2 are background now
    assert not O.bit_equal(want_big[0], want_small[0]).all()
    cfg = S.CONFIGS[2].with_size(128, 16)
    with ShadingContext(0) as ctx:
        ctx.set_pass(S.scene_pass(cfg))
        ctx.shade(S.build_gbuffer(cfg, gpu))
        stats, kernel = ctx.pass_stats(), ctx.last_kernel()
        assert stats["geometry_pixels"] == 128 * 16 and kernel
        at = Attributes.from_host(attrs, ids, gpu)
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        torch.cuda.synchronize()
        ctx.set_materials(big_m, big_t)
        outs = []
        for k in range(6):
            outs.append(("big", ctx.resolve(at, R.LINEAR, stream=(s1, s2)[k % 2])))
        ctx.set_materials(small_m, small_t, stream=s1)  # the big table is released after the queued resolves
        for k in range(6):
            outs.append(("small", ctx.resolve(at, R.LINEAR, stream=(s2, s1)[k % 2])))
        assert ctx.pass_stats() == stats and ctx.last_kernel() == kernel
        assert ctx.last_kernel(s1) == kernel and ctx.pass_stats(s2) == stats
        torch.cuda.synchronize()
        for k, (which, (gb, cov)) in enumerate(outs):
            want = want_big if which == "big" else want_small
            assert O.bit_equal(gb.planes.cpu().numpy(), want[0]).all(), (k, which)
            assert O.bit_equal(gb.opacity.cpu().numpy(), want[1]).all(), (k, which)
            assert np.array_equal(cov.cpu().numpy(), want[2]), (k, which)


def _raw_set_materials(ctx, mats, descs, n_materials=None):
    m = (N.MaterialDesc * max(len(mats), 1))(*[x.to_c() for x in mats])
    d = (N.TextureDesc * max(len(descs), 1))(*descs)
    return N.lib().pbr_set_materials(ctx.handle, m, len(mats) if n_materials is None else n_materials, d, len(descs),
                                     None)


def test_argument_errors(gpu):
    rng = np.random.default_rng(1)
    good = np.ascontiguousarray(rng.integers(0, 256, (4, 4, 3), dtype=np.uint8))

    def desc(t, w=None, h=None, c=None):
        d = N.TextureDesc()
        d.texels, d.height, d.width, d.channels = t.ctypes.data, t.shape[0], t.shape[1], t.shape[2]
        if w is not None:
            d.width = w
        if h is not None:
            d.height = h
        if c is not None:
            d.channels = c
        return d

    attrs, ids = shading_attributes(4, 16, 1, 1)
    with ShadingContext(0) as ctx:
        at = Attributes.from_host(attrs, ids, gpu)
        with pytest.raises(N.PbrError) as e:  # before pbr_set_materials
            ctx.resolve(at)
        assert e.value.status == N.PBR_ERR_NOT_READY
        inv = N.PBR_ERR_INVALID_ARGUMENT
        flagged = lambda slot, idx: Material(flags=1 << (slot if slot < 5 else 5),
                                             tex=tuple(idx if k == slot else -1 for k in range(6)))
        for slot in range(6):  # every flag: slot -1, slot == n_textures, slot beyond
            assert _raw_set_materials(ctx, [flagged(slot, -1)], [desc(good)]) == inv, slot
            assert _raw_set_materials(ctx, [flagged(slot, 1)], [desc(good)]) == inv, slot
            assert _raw_set_materials(ctx, [flagged(slot, 0)], []) == inv, slot
            assert _raw_set_materials(ctx, [flagged(slot, 0)], [desc(good)]) == 0, slot
        for c in (0, 2, 5):  # channels not in {1, 3, 4}, also under an .rgb slot
            assert _raw_set_materials(ctx, [Material()], [desc(good, c=c)]) == inv, c
            assert _raw_set_materials(ctx, [flagged(0, 0)], [desc(good, c=c)]) == inv, c
        for w, h in ((0, 4), (4, 0), (-1, 4), (4, -3)):  # non-positive sizes
            assert _raw_set_materials(ctx, [Material()], [desc(good, w=w, h=h)]) == inv, (w, h)
        many = (N.MaterialDesc * 0xFFFF)()
        assert N.lib().pbr_set_materials(ctx.handle, many, 0xFFFF, None, 0, None) == inv  # id 0xFFFF is NONE
        assert N.lib().pbr_set_materials(ctx.handle, many, 0xFFFE, None, 0, None) == 0
        assert N.lib().pbr_set_materials(ctx.handle, many, -1, None, 0, None) == inv
        assert _raw_set_materials(ctx, [Material(flags=1 << 6)], []) == inv  # unknown flag bit
        # the failed calls left the last good table in place; resolve-side argument errors
        ctx.set_materials([Material()], [])
        ctx.resolve(at)
        with pytest.raises(N.PbrError) as e:
            ctx.resolve(at, filter=2)
        assert e.value.status == inv
        a, t = at.to_c(), N.GBufferTargets()
        assert N.lib().pbr_resolve_materials(ctx.handle, a, t, 0, None) == inv  # NULL target planes
        a.row_stride = a.width - 1
        assert N.lib().pbr_resolve_materials(ctx.handle, a, t, 0, None) == inv
        torch.cuda.synchronize()


def test_bounds_checked_build_is_clean_and_equal(tmp_path, gpu, table, frames):
    """One case of the random-attribute test under _lib/debug_bounds/libpbrshade.so in a fresh child process
    (PBR_LIB_PATH): the result equals the restatement and no index class -- attribute reads, plane stores, coverage,
    table and texels -- is flagged."""
    if not os.path.exists(C.DEBUG_LIB):
        pytest.skip("bounds-checked build not built (make -C physically_based_renderer_amd/csrc debug-bounds)")
    out = tmp_path / "resolve_dbg.npz"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "resolve_cases.py"), str(out)],
                       env={**os.environ, "PBR_LIB_PATH": C.DEBUG_LIB}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)  # numeric and unicode arrays only: allow_pickle stays False
    assert str(z["flavor"]) == "debug_bounds" and str(z["sources_sha"]) == N.kernel_sources_sha()  # of this checkout
    assert (z["bounds"] < 0).all(), f"bounds violations (gbuffer/output/coverage/texel/light/lds): {z['bounds']}"
    attrs, ids = frames["70x3"]
    for name, filt in (("point_71", R.POINT), ("linear_70", R.LINEAR)):
        got = (z[name + "__planes"], z[name + "__opacity"], z[name + "__coverage"])
        check(got, expected(table, "70x3", attrs, ids, filt), 70, "debug-bounds " + name)


def test_native_driver_device_resolve_writes_the_same_frame(tmp_path, gpu):
    """pbr_render --config 4 --width 192 --height 128 --dump with and without --device-resolve: byte-identical."""
    exe = str(tmp_path / "pbr_render")
    lib_dir = os.path.dirname(N.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "pbr_render.cpp"), "-L", lib_dir, "-lpbrshade", "-lrccl", "-lz",
           f"-Wl,-rpath,{lib_dir}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dumps = []
    for extra in ([], ["--device-resolve"]):
        dump = str(tmp_path / f"frame{len(extra)}.bin")
        r = subprocess.run([exe, "--config", "4", "--width", "192", "--height", "128", "--dump", dump, *extra],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        dumps.append(open(dump, "rb").read())
    assert len(dumps[0]) == 16 + 192 * 128 * 16 and dumps[0] == dumps[1]
