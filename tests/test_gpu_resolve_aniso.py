"""pbr_resolve_materials_aniso on the GPU (material_resolve.h; DESIGN.md §11, "Anisotropic filter"): the anisotropic
resolve is held, bit for bit (oracle.bit_equal) in the 15 planes, opacity and coverage, to the numpy restatement of
tests/resolve_aniso_reference.py, which tests/test_resolve_aniso_host.py holds to the rule. Compared the way
tests/test_gpu_resolve_mip.py compares; the frames are 70 x 37 (a 64-wide tile and six more columns, odd width and
height, five tile rows) unless a case needs the 256 x 64 one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resolve_aniso_cases as AC
import resolve_aniso_reference as RA
import resolve_cases as C
import resolve_mip_cases as MC
import resolve_mip_reference as RM
from conftest import ROOT, oracle_pass_from_constants
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import envmap
from physically_based_renderer_amd import scenes as S
from physically_based_renderer_amd.renderer import Attributes, Draw, Material, Mesh, PassConstants, ShadingContext

pytestmark = pytest.mark.gpu

F = np.float32
ALL_FLAGS = 7  # MC.table(): every flag, every map another size
H, W = MC.SHAPES["70x37"]


def check(got, want, w, what):
    """Planes, opacity and coverage bit for bit on the frame's w columns; the padding columns of a strided canvas keep
    the canvas's sentinel."""
    (planes, opacity, cov), (eplanes, eopacity, ecov) = got, want
    for i, name in enumerate(N.PLANE_NAMES):
        eq = O.bit_equal(planes[i][:, :w], eplanes[i][:, :w])
        assert eq.all(), f"{what}: plane {name} differs at {np.argwhere(~eq)[:4].tolist()}"
    eq = O.bit_equal(opacity[:, :w], eopacity[:, :w])
    assert eq.all(), f"{what}: opacity differs at {np.argwhere(~eq)[:4].tolist()}"
    assert np.array_equal(cov[:, :w], ecov[:, :w]), f"{what}: coverage"
    assert (planes[:, :, w:] == C.SENTINEL).all() and (opacity[:, w:] == C.SENTINEL).all()
    assert (cov[:, w:] == C.SENTINEL_U8).all()


@pytest.fixture(scope="module")
def table():
    return MC.table()


@pytest.fixture(scope="module")
def chains(table):
    return [RM.build_mips(t) for t in table[1]]


@pytest.fixture(scope="module")
def ctx(gpu, table):
    c = ShadingContext(0)
    c.set_materials(*table)
    c.generate_mips()
    yield c
    c.close()


def want_of(table, chains, attrs, ids, m, bias=0.0):
    return RA.resolve_aniso(attrs, ids, table[0], table[1], m, bias, chains=chains)


def counts(table, chains, attrs, ids, texture, m, bias=0.0):
    """(N, lod) of one texture of the table over the frame."""
    d = RM.footprints(attrs[12], attrs[13], ids)
    t = table[1][texture]
    n, _, _, _, lod = RA.lod(*d, t.shape[1], t.shape[0], len(chains[texture]), bias, m)
    return n, lod


# ---- max_anisotropy 1 and pixels of one tap: the trilinear and the linear filter -----------------------------------

@pytest.mark.parametrize("bias", [0.0, 1.5])
@pytest.mark.parametrize("stride", [70, 71])
def test_max_anisotropy_1_equals_resolve_mip_on_the_device(ctx, table, chains, stride, bias):
    """The special UVs with valid partners, every material, background ids: with one tap allowed every plane is
    ctx.resolve_mip's, and the restatement's."""
    attrs, ids = MC.special_attributes(H, W, len(table[0]), seed=W)
    got = AC.device_resolve_aniso(ctx, attrs, ids, 1, bias, stride)
    check(got, MC.device_resolve_mip(ctx, attrs, ids, bias, stride), W, f"M 1 against resolve_mip, bias {bias}")
    check(got, want_of(table, chains, attrs, ids, 1, bias), W, f"M 1 stride {stride} bias {bias}")


@pytest.mark.parametrize("shape", list(MC.SHAPES))
def test_checkerboard_of_ids_equals_the_linear_filter(ctx, table, chains, shape):
    """Ids alternate pixel by pixel: every partner is invalid, every footprint +0, N = 1 and lod = 0 whatever M: the
    kernel must write what ctx.resolve(filter=LINEAR) writes."""
    h, w = MC.SHAPES[shape]
    attrs, _ = C.attributes(h, w, len(table[0]), seed=w + 1)
    ids = C.checker_ids(h, w, len(table[0]))
    got = AC.device_resolve_aniso(ctx, attrs, ids, 8, 0.0)
    check(got, C.device_resolve(ctx, attrs, ids, N.PBR_FILTER_LINEAR), w, f"{shape} checker against LINEAR")
    check(got, want_of(table, chains, attrs, ids, 8), w, f"{shape} checker")


# ---- tap counts ------------------------------------------------------------------------------------------------------

# the frame in five column bands of 14, one material each: diffuse alone over the 64x64, 256x1, 5x3 and 3x7 chain
# textures, and the normal map alone over the 16x32 one
BAND_MATERIALS = (13, 15, 11, 17, 5)


def band_ids(h, w):
    ids = np.empty((h, w), np.uint16)
    for k, m in enumerate(BAND_MATERIALS):
        ids[:, 14 * k:14 * (k + 1)] = m
    return ids


@pytest.mark.parametrize("major", ["x", "y"])
@pytest.mark.parametrize("m", [2, 8, 16])
def test_ramps_of_k_to_1_texels(ctx, table, chains, m, major):
    """k texels of the 64 x 64 map per pixel along one axis and 1 along the other, k through and past M: that map takes
    min(k, M) taps exactly; the other four textures see other ratios of the same ramp."""
    ids = band_ids(H, W)
    inner = np.zeros((H, W), bool)
    inner[:H - 1, 0:14] = True  # the 64 x 64 band without the last row (odd height: no vertical partner there)
    for k in (1, 2, 3, 5, 8, 9, 16, 17):
        long, short = k / 64.0, 1.0 / 64.0
        attrs = MC.ramp_attributes(H, W, long if major == "x" else short, short if major == "x" else long, u0=0.125,
                                   v0=-0.5)
        n, _ = counts(table, chains, attrs, ids, 2, m)
        assert (n[inner] == min(k, m)).all(), (k, m)
        got = AC.device_resolve_aniso(ctx, attrs, ids, m)
        check(got, want_of(table, chains, attrs, ids, m), W, f"ramp {major} {k}:1 M {m}")


def test_one_pixel_takes_another_tap_count_per_map(ctx, table, chains):
    """Material 7, every map another size, under 4 : 1 texels of the 64 x 64 maps: 4 taps there and on the 128 x 128 map,
    2 on the 16 x 32 map, M on the 256 x 1 map."""
    ids = np.full((H, W), ALL_FLAGS, np.uint16)
    attrs = MC.ramp_attributes(H, W, 4.0 / 64, 1.0 / 64, u0=0.125)
    inner = (slice(0, H - 1), slice(0, W))
    per_map = {t: counts(table, chains, attrs, ids, t, 8)[0][inner] for t in (5, 7, 8, 2, 3)}
    assert (per_map[5] == 4).all() and (per_map[8] == 4).all() and (per_map[2] == 4).all()
    assert (per_map[7] == 2).all() and (per_map[3] == 8).all()
    for bias in (0.0, 0.25):
        got = AC.device_resolve_aniso(ctx, attrs, ids, 8, bias)
        check(got, want_of(table, chains, attrs, ids, 8, bias), W, f"material 7, bias {bias}")


@pytest.mark.parametrize("shape,stride", [("70x37", 70), ("70x37", 71), ("256x64", 256)])
@pytest.mark.parametrize("waves", ["one-material", "mixed"])
def test_every_quad_its_own_footprint(ctx, table, chains, waves, shape, stride):
    """Random base UV and derivatives per 2 x 2 quad: tap counts from 1 to 16 side by side in one wave, the trip count
    of the tap loop differs from lane to lane and from map to map; under one material per wave (the wave-uniform record
    path) and under a material per quad (the per-lane path)."""
    h, w = MC.SHAPES[shape]
    attrs = AC.quad_attributes(h, w, seed=w + 3)
    if waves == "mixed":
        ids = AC.quad_ids(h, w, AC.TEXTURED, seed=w + 4)
    else:
        ids = np.full((h, w), ALL_FLAGS, np.uint16)
        ids[(np.arange(h)[:, None] * 5 + np.arange(w)[None, :] * 3) % 29 == 0] = N.PBR_MATERIAL_NONE
    n, lod = counts(table, chains, attrs, np.full((h, w), ALL_FLAGS, np.uint16), 5, 16)
    first_wave = n[0:2, 0:64]
    assert set(range(1, 17)) <= set(first_wave.ravel().tolist()), sorted(set(first_wave.ravel().tolist()))
    assert (lod > 0).any() and (lod == 0).any()
    for m, bias in ((16, 0.0), (8, 0.5)):
        got = AC.device_resolve_aniso(ctx, attrs, ids, m, bias, stride)
        check(got, want_of(table, chains, attrs, ids, m, bias), w, f"quads {waves} {shape} stride {stride} M {m}")


@pytest.mark.parametrize("m", [8, 16])
@pytest.mark.parametrize("stride", [70, 71])
def test_special_uvs_with_valid_partners(ctx, table, chains, stride, m):
    """NaN, +-inf, 3e9, negative and texel-edge UVs with a material per quad: footprints, tap coordinates and tap counts
    come out of NaN and inf; non-finite tap coordinates go through wrap_index as any UV does."""
    attrs, ids = MC.special_attributes(H, W, len(table[0]), seed=W)
    d = RM.footprints(attrs[12], attrs[13], ids)
    assert np.isnan(d[0]).any() and np.isinf(d[0]).any()
    for bias in (0.0, 0.75):
        got = AC.device_resolve_aniso(ctx, attrs, ids, m, bias, stride)
        check(got, want_of(table, chains, attrs, ids, m, bias), W, f"special M {m} stride {stride} bias {bias}")


def test_zero_minor_axis_takes_every_tap(ctx, table, chains):
    """Rows of constant UV (u and v change from row to row only), then columns of constant UV: the minor axis is +0, the
    major one is not, N = M; and a frame of one UV: both zero, N = 1."""
    ids = np.full((H, W), ALL_FLAGS, np.uint16)
    inner = (slice(0, H - 1), slice(0, W))
    for m in (8, 16):
        attrs = MC.ramp_attributes(H, W, 0.0, 3.0 / 64, u0=0.3)
        assert (counts(table, chains, attrs, ids, 5, m)[0][inner] == m).all()
        check(AC.device_resolve_aniso(ctx, attrs, ids, m), want_of(table, chains, attrs, ids, m), W, f"rows M {m}")
        attrs = MC.ramp_attributes(H, W, 0.5 / 64, 0.0, v0=0.3)
        assert (counts(table, chains, attrs, ids, 5, m)[0] == m).all()
        check(AC.device_resolve_aniso(ctx, attrs, ids, m), want_of(table, chains, attrs, ids, m), W, f"columns M {m}")
    attrs = MC.ramp_attributes(H, W, 0.0, 0.0, u0=0.3, v0=0.7)
    assert (counts(table, chains, attrs, ids, 5, 16)[0] == 1).all()
    got = AC.device_resolve_aniso(ctx, attrs, ids, 16)
    check(got, want_of(table, chains, attrs, ids, 16), W, "one UV")
    check(got, C.device_resolve(ctx, attrs, ids, N.PBR_FILTER_LINEAR), W, "one UV against LINEAR")


def test_biases_below_0_and_beyond_the_last_level(ctx, table, chains):
    ids = np.full((H, W), ALL_FLAGS, np.uint16)
    attrs = MC.ramp_attributes(H, W, 24.0 / 64, 2.0 / 64)   # 12 : 1: N = 8 at M = 8, lod 0.5 log2(576 / 64) + bias
    for bias in (-1.5, -40.0, 40.0, 2.25):
        got = AC.device_resolve_aniso(ctx, attrs, ids, 8, bias)
        check(got, want_of(table, chains, attrs, ids, 8, bias), W, f"bias {bias}")


def test_row_bands_that_start_on_even_rows_equal_the_frame(ctx, table):
    """The band rule of the trilinear call: quads are aligned to the call's row 0."""
    attrs = AC.quad_attributes(H, W, seed=9)
    ids = AC.quad_ids(H, W, AC.TEXTURED, seed=10)
    ids[8:] = C.uniform_ids(H, W, len(table[0]))[8:]
    full = AC.device_resolve_aniso(ctx, attrs, ids, 8, 0.25)
    for r0, r1 in ((0, 4), (4, 6), (6, 36), (36, 37), (10, 37)):
        band = AC.device_resolve_aniso(ctx, attrs, ids, 8, 0.25, rows=(r0, r1))
        for b, f in zip(band, full):
            inside, outside = b[..., r0:r1, :], np.delete(b, np.s_[r0:r1], axis=-2)
            if b.dtype == np.uint8:
                assert np.array_equal(inside, f[..., r0:r1, :]) and (outside == C.SENTINEL_U8).all(), (r0, r1)
            else:
                assert O.bit_equal(inside, f[..., r0:r1, :]).all() and (outside == C.SENTINEL).all(), (r0, r1)


# ---- lifetime and ordering ---------------------------------------------------------------------------------------------

def test_not_ready_and_argument_errors(gpu, table):
    attrs = MC.ramp_attributes(4, 16, 0.1, 0.1)
    ids = np.zeros((4, 16), np.uint16)
    with ShadingContext(0) as ctx:
        at = Attributes.from_host(attrs, ids, gpu)

        def status(call):
            with pytest.raises(N.PbrError) as e:
                call()
            return e.value.status

        assert status(lambda: ctx.resolve_aniso(at)) == N.PBR_ERR_NOT_READY       # before pbr_set_materials
        ctx.set_materials(*table)
        assert status(lambda: ctx.resolve_aniso(at)) == N.PBR_ERR_NOT_READY       # before pbr_generate_mips
        ctx.generate_mips()
        ctx.resolve_aniso(at)
        for m in (1, 16):
            ctx.resolve_aniso(at, m)
        for bad in (0, 17, -1):
            assert status(lambda: ctx.resolve_aniso(at, bad)) == N.PBR_ERR_INVALID_ARGUMENT
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert status(lambda: ctx.resolve_aniso(at, 8, bad)) == N.PBR_ERR_INVALID_ARGUMENT
        a, t = at.to_c(), N.GBufferTargets()
        assert N.lib().pbr_resolve_materials_aniso(ctx.handle, a, t, 0.0, 8, None) == N.PBR_ERR_INVALID_ARGUMENT  # NULL planes
        a.row_stride = a.width - 1
        assert N.lib().pbr_resolve_materials_aniso(ctx.handle, a, t, 0.0, 8, None) == N.PBR_ERR_INVALID_ARGUMENT
        ctx.set_materials(*table)                                                  # a new table: the chains are gone
        assert status(lambda: ctx.resolve_aniso(at)) == N.PBR_ERR_NOT_READY
        assert status(lambda: ctx.resolve_aniso(at, 0)) == N.PBR_ERR_INVALID_ARGUMENT
        ctx.generate_mips()
        gb, cov = ctx.resolve_aniso(at)
        torch.cuda.synchronize()
        assert (cov.cpu().numpy() == 1).all()


def test_tables_swapped_between_queued_calls_on_two_streams(gpu, table, chains):
    """resolve_aniso calls queued on two streams, set_materials + generate_mips of another table in between, more
    calls: each call sees its own table and chains (the call is a reader of both resources, as resolve_mip)."""
    big_m, big_t = table
    rng = np.random.default_rng(22)
    small_t = [rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)]
    small_m = [Material(flags=C.D, tex=(0, -1, -1, -1, -1, -1)), Material(roughness=0.2)] + \
              [Material(flags=C.D | C.NM, tex=(0, -1, -1, -1, 0, -1))] * (len(big_m) - 2)
    h, w = 64, 128
    attrs = MC.ramp_attributes(h, w, 6.5 / 64, 1.5 / 64)
    ids = C.uniform_ids(h, w, len(big_m))
    want_big = want_of(table, chains, attrs, ids, 8, 0.5)
    want_small = RA.resolve_aniso(attrs, ids, small_m, small_t, 8, 0.5)
    assert not O.bit_equal(want_big[0], want_small[0]).all()
    with ShadingContext(0) as ctx:
        at = Attributes.from_host(attrs, ids, gpu)
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        torch.cuda.synchronize()
        ctx.set_materials(big_m, big_t)
        ctx.generate_mips()
        outs = [("big", ctx.resolve_aniso(at, 8, 0.5, stream=(s1, s2)[k % 2])) for k in range(6)]
        ctx.set_materials(small_m, small_t, stream=s1)  # the big table and its chains are released after the queued calls
        ctx.generate_mips(stream=s2)
        outs += [("small", ctx.resolve_aniso(at, 8, 0.5, stream=(s2, s1)[k % 2])) for k in range(6)]
        ctx.set_materials(big_m, big_t, stream=s2)
        ctx.generate_mips(stream=s1)
        outs += [("big", ctx.resolve_aniso(at, 8, 0.5, stream=(s1, s2)[k % 2])) for k in range(2)]
        torch.cuda.synchronize()
        for k, (which, (gb, cov)) in enumerate(outs):
            want = want_big if which == "big" else want_small
            assert O.bit_equal(gb.planes.cpu().numpy(), want[0]).all(), (k, which)
            assert O.bit_equal(gb.opacity.cpu().numpy(), want[1]).all(), (k, which)
            assert np.array_equal(cov.cpu().numpy(), want[2]), (k, which)


def test_bounds_checked_build_is_clean_and_equal(tmp_path, gpu):
    """resolve_aniso_cases.bounds_cases() under _lib/debug_bounds/libpbrshade.so in a fresh child process
    (PBR_LIB_PATH): no index class is flagged -- slots, level table, both texel buffers are class "texel" -- and the
    results equal the restatement."""
    if not os.path.exists(C.DEBUG_LIB):
        pytest.skip("bounds-checked build not built (make -C physically_based_renderer_amd/csrc debug-bounds)")
    out = tmp_path / "resolve_aniso_dbg.npz"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "resolve_aniso_cases.py"), str(out)],
                       env={**os.environ, "PBR_LIB_PATH": C.DEBUG_LIB}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)  # numeric and unicode arrays only: allow_pickle stays False
    assert str(z["flavor"]) == "debug_bounds" and str(z["sources_sha"]) == N.kernel_sources_sha()  # of this checkout
    assert (z["bounds"] < 0).all(), f"bounds violations (gbuffer/output/coverage/texel/light/lds): {z['bounds']}"
    mats, texs, cases = AC.bounds_cases()
    for name, attrs, ids, m, bias, stride in cases:
        got = (z[name + "__planes"], z[name + "__opacity"], z[name + "__coverage"])
        assert attrs.shape[2] == (71 if name.startswith("odd") else 70) and got[0].shape[2] == stride
        check(got, RA.resolve_aniso(attrs, ids, mats, texs, m, bias), attrs.shape[2], "debug-bounds " + name)


# ---- end to end ---------------------------------------------------------------------------------------------------------

def floor_mesh(half_width, depth, tiles):
    """A quad on y = 0 from z = 0 to z = depth, its UV tiled `tiles` times per unit; front face up (left-handed)."""
    x, z = half_width, depth
    v = np.zeros((4, 14), np.float32)
    v[:, 0:3] = [(-x, 0, 0), (x, 0, 0), (x, 0, z), (-x, 0, z)]
    v[:, 3:6] = (0, 1, 0)
    v[:, 6:9] = (1, 0, 0)
    v[:, 9:12] = (0, 0, -1)
    v[:, 12] = (v[:, 0] + x) * tiles
    v[:, 13] = (z - v[:, 2]) * tiles
    return Mesh(v, np.array([0, 3, 2, 0, 2, 1], np.uint32))


def floor_scene(width, height, opacity=1.0):
    rng = np.random.default_rng(8)
    texs = [rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), rng.integers(0, 256, (32, 32), dtype=np.uint8)]
    mats = [Material(flags=C.D | C.R_, metallic=0.1, opacity=opacity, tex=(0, -1, -1, 1, -1, -1))]
    view = S.look_at_view((0.0, 1.5, -1.0), (0.0, 0.8, 6.0), float(np.pi / 3), width, height)
    lights = np.zeros((3, 12), np.float32)
    lights[:, 0:3] = rng.uniform(0.5, 2.0, (3, 3))
    lights[:, 4:7] = [(0.3, -0.8, 0.5), (-0.5, -0.6, 0.2), (0.0, -1.0, 0.0)]
    pc = PassConstants(eye_pos_w=view.eye, num_dir_lights=3, lights_array=lights, ambient_light=(0.1, 0.1, 0.1),
                       flags=N.PBR_FLAG_F0_PLANE)
    return texs, mats, [floor_mesh(30.0, 90.0, 0.5)], [Draw(mesh=0, material=0, cull=1)], view, pc


def test_receding_floor_rasterise_resolve_aniso_shade(gpu):
    """A textured floor to the horizon at 128 x 48: rasterize -> resolve_aniso -> shade_frame. The resolved G-buffer
    equals the restatement on the rasterised planes; the floor's footprints are long along the view, so most of its
    pixels take more than one tap and some the full eight; the frame (sky pass on the resolved coverage) equals the
    oracle's on the restatement's planes bit for bit in exact mode, and no pixel is left unwritten."""
    Wf, Hf = 128, 48
    texs, mats, meshes, draws, view, pc = floor_scene(Wf, Hf)
    sky = envmap.procedural_sky_rgba16(128, 64)
    with ShadingContext(0) as ctx:
        ctx.set_meshes(meshes)
        ctx.set_materials(mats, texs)
        ctx.generate_mips()
        ctx.set_sky_map(sky)
        at = ctx.rasterize(draws, view)
        gb, cov = ctx.resolve_aniso(at, 8)
        mip_gb, _ = ctx.resolve_mip(at)
        torch.cuda.synchronize()
        planes, ids = at.planes.cpu().numpy()[:, :, :Wf], at.material.cpu().numpy().view(np.uint16)[:, :Wf]
        assert (ids == 0).mean() > 0.3 and (ids == N.PBR_MATERIAL_NONE).mean() > 0.1
        want = RA.resolve_aniso(planes, ids, mats, texs, 8, 0.0)
        n = RA.lod(*RM.footprints(planes[12], planes[13], ids), 64, 64, 7, 0.0, 8)[0][ids == 0]
        print(f"floor tap counts: {np.bincount(n, minlength=9)[1:].tolist()}")
        assert (n > 1).mean() > 0.5 and (n == 8).any()
        assert O.bit_equal(gb.planes.cpu().numpy(), want[0]).all()
        assert O.bit_equal(gb.opacity.cpu().numpy(), want[1]).all() and np.array_equal(cov.cpu().numpy(), want[2])
        assert not O.bit_equal(gb.planes.cpu().numpy(), mip_gb.planes.cpu().numpy()).all()
        ctx.set_pass(pc)
        out = torch.full((Hf, Wf, 4), O.UNTOUCHED_F32, dtype=torch.float32, device=gpu)
        frame = ctx.shade_frame(gb, out, coverage=cov).cpu().numpy()
    ref = O.shade_frame(list(want[0]), oracle_pass_from_constants(pc), pc.light_array(), None, sky, want[2],
                        O.OUTPUT_RGBA32F, n_threads=8)
    print(f"receding floor, anisotropic 8: bit-identical {O.bit_equal(frame, ref).mean():.6f}")
    assert not (frame == O.UNTOUCHED_F32).any()
    assert O.bit_equal(frame, ref).all()


def test_draw_transparent_with_max_anisotropy_equals_the_composed_calls(gpu):
    """One transparent layer (the floor at opacity 0.5) over a cleared frame: draw_transparent(max_anisotropy=8) against
    rasterize_layer -> resolve_aniso -> shade -> blend_layer called one by one; with mip_lod_bias the bias is passed
    on; without max_anisotropy the result is another (the existing paths are what they were)."""
    Wf, Hf = 128, 48
    texs, mats, meshes, draws, view, pc = floor_scene(Wf, Hf, opacity=0.5)
    with ShadingContext(0) as ctx:
        ctx.set_meshes(meshes)
        ctx.set_materials(mats, texs)
        ctx.generate_mips()
        ctx.set_pass(pc)

        def helper(**kw):
            depth = torch.ones((Hf, Wf), dtype=torch.float32, device=gpu)
            frame = torch.zeros((Hf, Wf, 4), dtype=torch.float32, device=gpu)
            done = ctx.draw_transparent(draws, view, depth, frame, **kw)
            torch.cuda.synchronize()
            return done, frame.cpu().numpy(), depth.cpu().numpy()

        def composed(resolve):
            depth = torch.ones((Hf, Wf), dtype=torch.float32, device=gpu)
            frame = torch.zeros((Hf, Wf, 4), dtype=torch.float32, device=gpu)
            attrs = Attributes(torch.empty((N.NUM_ATTRIBUTE_PLANES, Hf, Wf), dtype=torch.float32, device=gpu),
                               torch.empty((Hf, Wf), dtype=torch.int16, device=gpu))
            at, _ = ctx.rasterize_layer(draws, view, depth, None, 0, out=(attrs, depth))
            assert ctx.raster_layer_stats()["layer_fragments"] > 0
            gb, cov = resolve(at)
            shaded = ctx.shade(gb)
            ctx.blend_layer(shaded, gb.opacity, cov, frame, width=Wf, height=Hf)
            torch.cuda.synchronize()
            return frame.cpu().numpy(), depth.cpu().numpy()

        done, frame, depth = helper(max_anisotropy=8)
        want_frame, want_depth = composed(lambda at: ctx.resolve_aniso(at, 8, 0.0))
        assert done == (1, True)
        assert O.bit_equal(frame, want_frame).all() and O.bit_equal(depth, want_depth).all()
        assert (frame[..., 3] == 0.5).mean() > 0.3
        done, biased, _ = helper(max_anisotropy=8, mip_lod_bias=0.75)
        assert done == (1, True)
        assert O.bit_equal(biased, composed(lambda at: ctx.resolve_aniso(at, 8, 0.75))[0]).all()
        assert not O.bit_equal(biased, frame).all()
        done, trilinear, _ = helper(mip_lod_bias=0.0)
        assert done == (1, True)
        assert O.bit_equal(trilinear, composed(lambda at: ctx.resolve_mip(at, 0.0))[0]).all()
        assert not O.bit_equal(trilinear, frame).all()
