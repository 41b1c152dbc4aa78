"""pbr_generate_mips and pbr_resolve_materials_mip on the GPU (material_resolve.h; DESIGN.md §11, "Mip chains and the
trilinear filter"): the chains built on the device and the trilinear resolve are held, bit for bit (oracle.bit_equal)
in the 15 planes, opacity and coverage, to the numpy restatement of tests/resolve_mip_reference.py, which
tests/test_resolve_mip_host.py holds to the rules."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resolve_cases as C
import resolve_mip_cases as MC
import resolve_mip_reference as RM
import resolve_reference as R
from conftest import ROOT, oracle_pass_from_constants
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import envmap
from physically_based_renderer_amd import scenes as S
from physically_based_renderer_amd.renderer import Attributes, Draw, Material, Mesh, PassConstants, ShadingContext

pytestmark = pytest.mark.gpu

F = np.float32
ALL_FLAGS = 7  # MC.table(): every flag, every map another size


def check(got, want, w, what):
    """Planes, opacity and coverage bit for bit on the frame's w columns; the padding columns of a strided canvas and of
    `want` (another device result) are not compared beyond the canvas's sentinel."""
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


def want_of(table, chains, attrs, ids, bias):
    return RM.resolve_mip(attrs, ids, table[0], table[1], bias, chains=chains)


# ---- chain contents, read back through sampling ---------------------------------------------------------------------

@pytest.mark.parametrize("t", range(len(MC.CHAIN_TEXTURES)), ids=[c[0] for c in MC.CHAIN_TEXTURES])
def test_chain_contents_through_sampling(ctx, table, chains, t):
    """Two identical materials over the texture alternate pixel by pixel, so every partner is invalid and lod is the
    bias: for every level k, pixels on the centres of every texel of level k under bias k (the bilinear of level k
    alone) and k + 0.5 (levels k and k + 1 mixed; the last level clamps)."""
    h, w = MC.SHAPES["256x64"]
    ids = MC.alternate_ids(h, w, 9 + 2 * t, 10 + 2 * t)
    chain = chains[t]
    assert [(l.shape[1], l.shape[0]) for l in chain][0] == MC.CHAIN_TEXTURES[t][2:0:-1]
    for k, level in enumerate(chain):
        attrs = MC.texel_centre_attributes(h, w, level.shape[1], level.shape[0])
        for bias in (float(k), k + 0.5):
            got = MC.device_resolve_mip(ctx, attrs, ids, bias)
            check(got, want_of(table, chains, attrs, ids, bias), w, f"texture {t} level {k} bias {bias}")


# ---- resolve cases ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bias", [0.0, 0.75])
@pytest.mark.parametrize("shape,stride", [("70x37", 70), ("70x37", 71), ("256x64", 256)])
def test_random_attributes_equal_the_restatement(ctx, table, chains, shape, stride, bias):
    """resolve_cases.attributes with a material per quad over the special UVs (NaN, +-inf, 3e9, negative, texel edges:
    footprints come out NaN and inf): every material flag combination, background ids mixed in, random UVs elsewhere
    (large footprints: the last levels), a zero-length normal; odd width and height; stride 71 takes the scalar
    accesses, the even ones the paired."""
    h, w = MC.SHAPES[shape]
    attrs, ids = MC.special_attributes(h, w, len(table[0]), seed=w)
    assert (ids == N.PBR_MATERIAL_NONE).any() and set(range(len(table[0]))) <= set(ids.ravel().tolist())
    d = RM.footprints(attrs[12], attrs[13], ids)
    assert np.isnan(d[0]).any() and np.isinf(d[0]).any()
    got = MC.device_resolve_mip(ctx, attrs, ids, bias, stride)
    check(got, want_of(table, chains, attrs, ids, bias), w, f"{shape} stride {stride} bias {bias}")


@pytest.mark.parametrize("shape", list(MC.SHAPES))
def test_checkerboard_of_ids_equals_the_linear_filter(ctx, table, chains, shape):
    """Ids alternate pixel by pixel: every partner is invalid, lod is 0, and the trilinear kernel must write what
    ctx.resolve(filter=LINEAR) writes, bit for bit -- and what the restatement says."""
    h, w = MC.SHAPES[shape]
    attrs, _ = C.attributes(h, w, len(table[0]), seed=w + 1)
    ids = C.checker_ids(h, w, len(table[0]))
    got = MC.device_resolve_mip(ctx, attrs, ids, 0.0)
    linear = C.device_resolve(ctx, attrs, ids, N.PBR_FILTER_LINEAR)
    check(got, linear, w, f"{shape} checker against LINEAR")
    check(got, want_of(table, chains, attrs, ids, 0.0), w, f"{shape} checker")


@pytest.mark.parametrize("shape", list(MC.SHAPES))
def test_uniform_waves_equal_the_restatement(ctx, table, chains, shape):
    """One material per wave (64 x 2 pixels) with background pixels inside: the wave-uniform record path, under a smooth
    UV field whose footprint grows across the frame."""
    h, w = MC.SHAPES[shape]
    attrs = MC.ramp_attributes(h, w, 1.0 / 64, 1.0 / 128)
    attrs[12] = attrs[12] * attrs[12] * F(2.0)
    ids = C.uniform_ids(h, w, len(table[0]))
    for bias in (0.0, 0.5):
        got = MC.device_resolve_mip(ctx, attrs, ids, bias)
        check(got, want_of(table, chains, attrs, ids, bias), w, f"{shape} uniform bias {bias}")


def test_one_material_waves_and_mixed_waves_agree(ctx, table, chains):
    """The same pixels resolved by one-material waves and by mixed waves: a frame of material 7, and the same frame with
    one quad per wave given to material 1. Outside those quads the two results are equal bit for bit."""
    h, w = MC.SHAPES["256x64"]
    attrs = MC.ramp_attributes(h, w, 3.0 / 64, 5.0 / 64, u0=-0.3)
    uniform = np.full((h, w), ALL_FLAGS, np.uint16)
    mixed = uniform.copy()
    touched = np.zeros((h, w), bool)
    for y in range(0, h, 2):
        for x0 in range(0, w, 64):
            x = x0 + 2 * ((y // 2 * 7 + x0 // 64 * 3) % 32)
            mixed[y:y + 2, x:x + 2] = 1
            touched[y:y + 2, x:x + 2] = True
    a = MC.device_resolve_mip(ctx, attrs, uniform, 0.25)
    b = MC.device_resolve_mip(ctx, attrs, mixed, 0.25)
    check(a, want_of(table, chains, attrs, uniform, 0.25), w, "one-material waves")
    check(b, want_of(table, chains, attrs, mixed, 0.25), w, "mixed waves")
    assert O.bit_equal(a[0][:, ~touched], b[0][:, ~touched]).all() and O.bit_equal(a[1][~touched], b[1][~touched]).all()


RAMPS = [(axis, k) for axis in ("x", "y", "both") for k in range(4)]


@pytest.mark.parametrize("axis,k", RAMPS, ids=[f"{a}-{k}" for a, k in RAMPS])
def test_ramps_of_2_to_the_k_texels_per_pixel(ctx, table, chains, axis, k):
    """2^k texels of the 64 x 64 map per pixel in x only, in y only and in both, under the material whose maps all have
    another size: the 64 x 64 map sits exactly on level k, the others on their own levels (the lod is per texture)."""
    h, w = MC.SHAPES["70x37"]
    step = 2.0 ** k / 64.0
    attrs = MC.ramp_attributes(h, w, step if axis != "y" else 0.0, step if axis != "x" else 0.0, u0=0.125, v0=-0.5)
    ids = np.full((h, w), ALL_FLAGS, np.uint16)
    d = RM.footprints(attrs[12], attrs[13], ids)
    inner = (slice(0, h - 1), slice(0, w))  # the last row of an odd height has no vertical partner
    lods = {t: RM.lod(*d, table[1][t].shape[1], table[1][t].shape[0], len(chains[t]), 0.0)[3] for t in (5, 7, 8)}
    assert (lods[5][inner] == k).all()                      # 64 x 64 diffuse map
    assert (lods[8][inner] == min(k + 1, 7)).all()          # 128 x 128 metallic map: one level up
    if axis == "x":
        assert (lods[7][inner] == max(k - 2, 0)).all()      # 16 wide specular map: two levels down
    got = MC.device_resolve_mip(ctx, attrs, ids, 0.0)
    check(got, want_of(table, chains, attrs, ids, 0.0), w, f"ramp {axis} 2^{k}")


def test_r2_straddling_1_seam_and_biases(ctx, table, chains):
    """(a) a ramp in y whose step grows row pair by row pair through 1 texel per pixel of the 64 x 64 map: r2 just below,
    at and just above 1; (b) u wraps 1 -> 0 inside a quad: a footprint of almost the whole map, the last levels;
    (c) a negative bias under a minified ramp, (d) a bias beyond the last level: every texture at its 1 x 1 level."""
    h, w = MC.SHAPES["70x37"]
    ids = np.full((h, w), ALL_FLAGS, np.uint16)
    attrs = MC.ramp_attributes(h, w, 0.0, 0.0)
    one = F(1.0 / 64.0)
    steps = [np.nextafter(one, F(0)), one, np.nextafter(one, F(1)), one * F(1.0001), one * F(0.9999), one * F(1.5)]
    for y in range(0, h - 1, 2):
        attrs[13, y + 1] = attrs[13, y] + steps[(y // 2) % len(steps)]
    lod = RM.lod(*RM.footprints(attrs[12], attrs[13], ids), 64, 64, 7, 0.0)[3]
    assert (lod[:h - 1] == 0).any() and ((lod > 0) & (lod < 1e-3)).any() and (lod > 0.25).any()
    got = MC.device_resolve_mip(ctx, attrs, ids, 0.0)
    check(got, want_of(table, chains, attrs, ids, 0.0), w, "r2 straddling 1")

    attrs = MC.ramp_attributes(h, w, 1.0 / 256, 1.0 / 256, u0=0.99)
    attrs[12] = attrs[12] - np.floor(attrs[12])  # frac: the seam falls at x = 3, inside the quad of columns 2 and 3
    d = RM.footprints(attrs[12], attrs[13], ids)
    assert (d[0][:, 2] < -0.9).all() and (d[0][:, 4] > 0).all()
    got = MC.device_resolve_mip(ctx, attrs, ids, 0.0)
    check(got, want_of(table, chains, attrs, ids, 0.0), w, "u seam")

    attrs = MC.ramp_attributes(h, w, 8.0 / 64, 8.0 / 64)
    for bias in (-1.5, -40.0, 40.0):
        got = MC.device_resolve_mip(ctx, attrs, ids, bias)
        check(got, want_of(table, chains, attrs, ids, bias), w, f"bias {bias}")


def test_row_bands_that_start_on_even_rows_equal_the_frame(ctx, table):
    """Quads are aligned to the call's row 0: bands through offset pointers that start on an even frame row and have an
    even height or end with the (odd) frame equal the frame's rows; rows outside a band keep the canvas's sentinel."""
    h, w = MC.SHAPES["70x37"]
    attrs, ids = C.attributes(h, w, len(table[0]), seed=5)
    attrs[12:14, 8:] = MC.ramp_attributes(h, w, 0.013, 0.021)[12:14, 8:] ** 2
    ids[8:] = C.uniform_ids(h, w, len(table[0]))[8:]
    full = MC.device_resolve_mip(ctx, attrs, ids, 0.25)
    for r0, r1 in ((0, 4), (4, 6), (6, 36), (36, 37), (10, 37)):
        band = MC.device_resolve_mip(ctx, attrs, ids, 0.25, rows=(r0, r1))
        for b, f in zip(band, full):
            inside, outside = b[..., r0:r1, :], np.delete(b, np.s_[r0:r1], axis=-2)
            if b.dtype == np.uint8:
                assert np.array_equal(inside, f[..., r0:r1, :]) and (outside == C.SENTINEL_U8).all(), (r0, r1)
            else:
                assert O.bit_equal(inside, f[..., r0:r1, :]).all() and (outside == C.SENTINEL).all(), (r0, r1)


# ---- lifetime and ordering ----------------------------------------------------------------------------------------------

def test_not_ready_and_argument_errors(gpu, table):
    attrs = MC.ramp_attributes(4, 16, 0.1, 0.1)
    ids = np.zeros((4, 16), np.uint16)
    with ShadingContext(0) as ctx:
        at = Attributes.from_host(attrs, ids, gpu)

        def status(call):
            with pytest.raises(N.PbrError) as e:
                call()
            return e.value.status

        assert status(ctx.generate_mips) == N.PBR_ERR_NOT_READY           # before pbr_set_materials
        assert status(lambda: ctx.resolve_mip(at)) == N.PBR_ERR_NOT_READY
        ctx.set_materials(*table)
        ctx.resolve(at, R.LINEAR)
        assert status(lambda: ctx.resolve_mip(at)) == N.PBR_ERR_NOT_READY  # before pbr_generate_mips
        ctx.generate_mips()
        ctx.resolve_mip(at)
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert status(lambda: ctx.resolve_mip(at, bad)) == N.PBR_ERR_INVALID_ARGUMENT
        assert status(lambda: ctx.resolve(at, filter=2)) == N.PBR_ERR_INVALID_ARGUMENT  # not a value of `filter`
        a, t = at.to_c(), N.GBufferTargets()
        assert N.lib().pbr_resolve_materials_mip(ctx.handle, a, t, 0.0, None) == N.PBR_ERR_INVALID_ARGUMENT  # NULL planes
        a.row_stride = a.width - 1
        assert N.lib().pbr_resolve_materials_mip(ctx.handle, a, t, 0.0, None) == N.PBR_ERR_INVALID_ARGUMENT
        ctx.set_materials(*table)                                          # a new table: the chains are gone
        assert status(lambda: ctx.resolve_mip(at)) == N.PBR_ERR_NOT_READY
        ctx.resolve(at, R.LINEAR)
        ctx.generate_mips()
        ctx.generate_mips()                                                # again: the first chains are released
        ctx.resolve_mip(at)
        ctx.set_materials([], [])                                          # no texture at all
        ctx.generate_mips()
        gb, cov = ctx.resolve_mip(at)
        torch.cuda.synchronize()
        assert (cov.cpu().numpy() == 0).all()


def test_tables_swapped_between_queued_calls_on_two_streams(gpu, table, chains):
    """resolve_mip calls queued on two streams, set_materials + generate_mips of another table in between, more calls:
    each call sees its own table's chains. ctx.resolve gives the same before and after all of it."""
    big_m, big_t = table
    rng = np.random.default_rng(21)
    small_t = [rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)]
    small_m = [Material(flags=C.D, tex=(0, -1, -1, -1, -1, -1)), Material(roughness=0.2)] + \
              [Material(flags=C.D | C.NM, tex=(0, -1, -1, -1, 0, -1))] * (len(big_m) - 2)
    h, w = 128, 192
    attrs = MC.ramp_attributes(h, w, 2.5 / 64, 1.5 / 64)
    ids = C.uniform_ids(h, w, len(big_m))
    want_big = want_of(table, chains, attrs, ids, 0.5)
    want_small = RM.resolve_mip(attrs, ids, small_m, small_t, 0.5)
    assert not O.bit_equal(want_big[0], want_small[0]).all()
    with ShadingContext(0) as ctx:
        at = Attributes.from_host(attrs, ids, gpu)
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        torch.cuda.synchronize()
        ctx.set_materials(big_m, big_t)
        before = ctx.resolve(at, R.LINEAR)
        ctx.generate_mips()
        outs = [("big", ctx.resolve_mip(at, 0.5, stream=(s1, s2)[k % 2])) for k in range(6)]
        ctx.set_materials(small_m, small_t, stream=s1)  # the big table and its chains are released after the queued calls
        ctx.generate_mips(stream=s2)
        outs += [("small", ctx.resolve_mip(at, 0.5, stream=(s2, s1)[k % 2])) for k in range(6)]
        ctx.set_materials(big_m, big_t, stream=s2)
        ctx.generate_mips(stream=s1)
        outs += [("big", ctx.resolve_mip(at, 0.5, stream=(s1, s2)[k % 2])) for k in range(2)]
        after = ctx.resolve(at, R.LINEAR, stream=s1)
        torch.cuda.synchronize()
        for k, (which, (gb, cov)) in enumerate(outs):
            want = want_big if which == "big" else want_small
            assert O.bit_equal(gb.planes.cpu().numpy(), want[0]).all(), (k, which)
            assert O.bit_equal(gb.opacity.cpu().numpy(), want[1]).all(), (k, which)
            assert np.array_equal(cov.cpu().numpy(), want[2]), (k, which)
        assert O.bit_equal(before[0].planes.cpu().numpy(), after[0].planes.cpu().numpy()).all()
        assert O.bit_equal(before[0].planes.cpu().numpy(), R.resolve(attrs, ids, big_m, big_t, R.LINEAR)[0]).all()


def test_bounds_checked_build_is_clean_and_equal(tmp_path, gpu):
    """resolve_mip_cases.BOUNDS_RUNS (bounds_case() at 70 columns, bounds_case_odd_width() at 71) under
    _lib/debug_bounds/libpbrshade.so in a fresh child process (PBR_LIB_PATH):
    generation and resolve flag no index class -- slots, level table, both texel buffers are class "texel" -- and the
    result equals the restatement."""
    if not os.path.exists(C.DEBUG_LIB):
        pytest.skip("bounds-checked build not built (make -C physically_based_renderer_amd/csrc debug-bounds)")
    out = tmp_path / "resolve_mip_dbg.npz"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "resolve_mip_cases.py"), str(out)],
                       env={**os.environ, "PBR_LIB_PATH": C.DEBUG_LIB}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)  # numeric and unicode arrays only: allow_pickle stays False
    assert str(z["flavor"]) == "debug_bounds" and str(z["sources_sha"]) == N.kernel_sources_sha()  # of this checkout
    assert (z["bounds"] < 0).all(), f"bounds violations (gbuffer/output/coverage/texel/light/lds): {z['bounds']}"
    mats, texs, attrs, ids = MC.bounds_case()
    odd = MC.bounds_case_odd_width()
    assert [r[0] for r in MC.BOUNDS_RUNS[:2]] == ["bias0_71", "bias1.5_70"]
    for name, odd_width, bias, stride in MC.BOUNDS_RUNS:
        a, i = odd if odd_width else (attrs, ids)
        got = (z[name + "__planes"], z[name + "__opacity"], z[name + "__coverage"])
        assert got[0].shape[2] == stride
        check(got, RM.resolve_mip(a, i, mats, texs, bias), a.shape[2], "debug-bounds " + name)


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


def test_receding_floor_and_sphere_rasterise_resolve_mip_shade(gpu):
    """A textured floor to the horizon and a normal-mapped sphere at 256 x 64: rasterize -> resolve_mip -> shade_frame.
    The resolved G-buffer equals the restatement on the rasterised planes; the floor's lod spans at least three levels;
    the frame (sky pass on the resolved coverage) equals the oracle's on the restatement's planes bit for bit in exact
    mode, within 1e-5 in faithful mode, and no pixel is left unwritten."""
    W, H = 256, 64
    rng = np.random.default_rng(8)
    texs = [rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), rng.integers(0, 256, (32, 32), dtype=np.uint8),
            np.clip(rng.normal(128, 30, (64, 64, 3)), 0, 255).astype(np.uint8)]
    texs[2][..., 2] = 255  # a normal map that mostly points out
    mats = [Material(flags=C.D | C.R_, metallic=0.1, tex=(0, -1, -1, 1, -1, -1)),
            Material(diffuse_albedo=(0.9, 0.6, 0.2), metallic=0.8, roughness=0.35, flags=C.NM | C.D, tex=(0, -1, -1, -1, 2, -1))]
    meshes = [floor_mesh(30.0, 90.0, 0.5), S.uv_sphere(32, 16)]
    draws = [Draw(mesh=0, material=0, cull=1), Draw(mesh=1, material=1, world=S.translation(0.0, 1.0, 4.0))]
    view = S.look_at_view((0.0, 1.5, -1.0), (0.0, 0.8, 6.0), float(np.pi / 3), W, H)
    lights = np.zeros((3, 12), np.float32)
    lights[:, 0:3] = rng.uniform(0.5, 2.0, (3, 3))
    lights[:, 4:7] = [(0.3, -0.8, 0.5), (-0.5, -0.6, 0.2), (0.0, -1.0, 0.0)]
    pc = PassConstants(eye_pos_w=view.eye, num_dir_lights=3, lights_array=lights, ambient_light=(0.1, 0.1, 0.1),
                       flags=N.PBR_FLAG_F0_PLANE)
    sky = envmap.procedural_sky_rgba16(128, 64)
    with ShadingContext(0) as ctx:
        ctx.set_meshes(meshes)
        ctx.set_materials(mats, texs)
        ctx.generate_mips()
        ctx.set_sky_map(sky)
        at = ctx.rasterize(draws, view)
        gb, cov = ctx.resolve_mip(at)
        torch.cuda.synchronize()
        planes, ids = at.planes.cpu().numpy()[:, :, :W], at.material.cpu().numpy().view(np.uint16)[:, :W]
        assert (ids == 0).mean() > 0.3 and (ids == 1).mean() > 0.02 and (ids == N.PBR_MATERIAL_NONE).mean() > 0.1
        want = RM.resolve_mip(planes, ids, mats, texs, 0.0)
        lod = RM.lod(*RM.footprints(planes[12], planes[13], ids), 64, 64, 7, 0.0)[3][ids == 0]
        print(f"floor lod {lod.min():.3f} .. {lod.max():.3f}")
        assert lod.max() - lod.min() >= 3.0
        assert O.bit_equal(gb.planes.cpu().numpy(), want[0]).all()
        assert O.bit_equal(gb.opacity.cpu().numpy(), want[1]).all() and np.array_equal(cov.cpu().numpy(), want[2])
        ctx.set_pass(pc)
        out = torch.full((H, W, 4), O.UNTOUCHED_F32, dtype=torch.float32, device=gpu)
        frame = ctx.shade_frame(gb, out, coverage=cov).cpu().numpy()
        ref = O.shade_frame(list(want[0]), oracle_pass_from_constants(pc), pc.light_array(), None, sky, want[2],
                            O.OUTPUT_RGBA32F, n_threads=8)
        print(f"floor and sphere, trilinear: bit-identical {O.bit_equal(frame, ref).mean():.6f}")
        assert not (frame == O.UNTOUCHED_F32).any()
        assert O.bit_equal(frame, ref).all()
        pc.flags |= N.PBR_FLAG_FAITHFUL
        ctx.set_pass(pc)
        faithful = ctx.shade_frame(gb, coverage=cov).cpu().numpy()
    err = O.rel_err(faithful, ref).max()
    print(f"faithful max_rel {err:.3g}")
    assert err <= 1e-5
