"""pbr_rasterize_layer on the GPU (csrc/raster.h) and the transparent pass built on it
(ShadingContext.draw_transparent: layer -> resolve -> shade -> pbr_blend_layer). Every layer comparison is bit for bit
(oracle.bit_equal, NaN patterns equal) against the numpy restatement of tests/raster_layer_reference.py -- all 14 planes,
the material, depth and floor planes -- and every counter exactly, layer after layer until the empty one.
tests/test_raster_layer_host.py checks the restatement against the sequential depth-tested pass. A library without the
entry points fails every test here (the binding raises); none is skipped."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import blend_layer_reference as BR
import raster_alpha_reference as AR
import raster_cases as C
import raster_clip_cases as CC
import raster_layer_cases as LC
import raster_layer_reference as LR
import raster_reference as R
import resolve_reference as RR
from conftest import ROOT, oracle_pass_from_constants
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import envmap
from physically_based_renderer_amd import scenes as S
from physically_based_renderer_amd.renderer import Attributes, Draw, Material, ShadingContext

pytestmark = pytest.mark.gpu

ZERO_LAYER = dict.fromkeys(LR.LAYER_STAT_NAMES, 0)
ZERO_ALPHA = dict.fromkeys(AR.ALPHA_STAT_NAMES, 0)


@pytest.fixture(scope="module")
def ctx(gpu):
    c = ShadingContext(0)
    yield c
    c.close()


_expected = {}


def host_depth0(sc):
    return AR.rasterize(sc.meshes, sc.opaque, sc.view, [], [], sc.clip_near, alpha_test=False)[2]


def expected(name, frame):
    """(scene, d_0, the restatement's layers down to the empty one) of one case, computed once and shared."""
    if (name, frame) not in _expected:
        W, H = LC.FRAMES[frame]
        sc = LC.case(name, W, H)
        d0 = host_depth0(sc)
        _expected[(name, frame)] = (sc, d0, LR.peel(sc.meshes, sc.draws, sc.view, d0, sc.clip_near))
    return _expected[(name, frame)]


def check(got, counters, want, W, what, rows=None, pad_depth=C.SENTINEL, pad_prim=C.SENTINEL_ID, outside=None):
    """One device layer against a Layer of the restatement. ``outside``: (depth, prim) host planes the rows outside
    the band and the padding columns must still hold (default: the canvases' sentinels)."""
    planes, ids, depth, prim = got
    r0, r1 = (0, planes.shape[1]) if rows is None else rows
    for k in range(14):
        eq = O.bit_equal(planes[k][r0:r1, :W], want.planes[k][r0:r1])
        assert eq.all(), f"{what}: plane {k} differs at {np.argwhere(~eq)[:4].tolist()}"
    eq = ids[r0:r1, :W] == want.material[r0:r1]
    assert eq.all(), f"{what}: material differs at {np.argwhere(~eq)[:4].tolist()}"
    eq = O.bit_equal(depth[r0:r1, :W], want.depth[r0:r1])
    assert eq.all(), f"{what}: depth differs at {np.argwhere(~eq)[:4].tolist()}"
    eq = prim[r0:r1, :W] == want.prim[r0:r1]
    assert eq.all(), f"{what}: floor differs at {np.argwhere(~eq)[:4].tolist()}"
    if rows is None and counters is not None:
        stats, clip, layer, alpha = counters
        assert stats == want.stats, f"{what}: stats {stats} != {want.stats}"
        assert clip == want.clip, f"{what}: clip stats {clip} != {want.clip}"
        assert layer == want.layer, f"{what}: layer stats {layer} != {want.layer}"
        assert alpha == ZERO_ALPHA
    # the padding columns of a strided canvas, and the rows outside a band, are never written
    out = np.ones(planes.shape[1], bool)
    out[r0:r1] = False
    assert (planes[:, :, W:] == C.SENTINEL).all() and (ids[:, W:] == C.SENTINEL_ID).all()
    assert (planes[:, out] == C.SENTINEL).all() and (ids[out] == C.SENTINEL_ID).all()
    if outside is None:
        assert (depth[:, W:] == pad_depth).all() and (prim[:, W:] == np.uint32(pad_prim)).all()
        assert (depth[out] == pad_depth).all() and (prim[out] == np.uint32(pad_prim)).all()
    else:
        assert O.bit_equal(depth[:, W:], outside[0][:, W:]).all() and (prim[:, W:] == outside[1][:, W:]).all()
        assert O.bit_equal(depth[out], outside[0][out]).all() and (prim[out] == outside[1][out]).all()


def peel_on_device(ctx, sc, d0, layers, W, stride, alias, what):
    """Every layer of the restatement, the empty one included, on the device: separate planes fed the previous
    layer's outputs, or (``alias``) one depth plane and one floor plane updated in place."""
    ctx.set_meshes(sc.meshes)
    depth = LC.device_depth0(ctx, sc, stride)
    torch.cuda.synchronize()
    assert O.bit_equal(depth.cpu().numpy()[:, :W], d0).all(), f"{what}: the opaque depth"
    prim = torch.zeros((depth.shape[0], stride), dtype=torch.int32, device=depth.device) if alias else None
    for k, want in enumerate(layers):
        got, counters = LC.device_layer(ctx, sc, depth, prim, stride=stride, alias=alias)
        host = LC.to_host(got)
        if alias:  # the padding columns keep what the planes held before the call: d_0's padding and zeros
            check(host, counters, want, W, f"{what} layer {k}", pad_depth=C.SENTINEL, pad_prim=0)
        else:
            check(host, counters, want, W, f"{what} layer {k}")
        depth, prim = got[2], got[3]
    assert layers[-1].layer == ZERO_LAYER and all(l.layer["layer_fragments"] > 0 for l in layers[:-1])


@pytest.mark.parametrize("frame", list(LC.FRAMES))
@pytest.mark.parametrize("name", LC.CASES)
def test_case_peels_to_the_restatement(ctx, name, frame):
    """Every case in both frames, layer after layer until the empty one: into an odd row stride (width + 1: the scalar
    stores) with separate in and out planes and prim_in NULL for the first layer, and into an even one (width: the
    paired stores) with the depth plane aliasing depth_in, prim_out aliasing prim_in and an all-zero first floor."""
    W, H = LC.FRAMES[frame]
    sc, d0, layers = expected(name, frame)
    print(name, frame, "layers", len(layers) - 1, [l.layer["layer_fragments"] for l in layers], layers[0].stats)
    if LC.CHAINS[name] is not None:
        assert len(layers) - 1 == LC.CHAINS[name]
    peel_on_device(ctx, sc, d0, layers, W, W + 1, False, f"{name} {frame} separate")
    peel_on_device(ctx, sc, d0, layers, W, W, True, f"{name} {frame} aliased")


@pytest.mark.parametrize("stride_pad", [0, 1])
def test_aliased_and_null_floor_variants_agree(ctx, stride_pad):
    """intersecting at 70x37: the four combinations of (separate, aliased) and, for the first layer, (prim_in NULL,
    an all-zero plane) give the same planes, in both store layouts."""
    W, H = LC.FRAMES["70x37"]
    sc, d0, layers = expected("intersecting", "70x37")
    stride = W + stride_pad
    ctx.set_meshes(sc.meshes)
    zeros = torch.zeros((H, stride), dtype=torch.int32, device="cuda")
    for prim_in in (None, zeros):
        depth = LC.device_depth0(ctx, sc, stride)
        got, counters = LC.device_layer(ctx, sc, depth, prim_in, stride=stride)
        check(LC.to_host(got), counters, layers[0], W, f"separate, floor {prim_in is not None}")
    depth = LC.device_depth0(ctx, sc, stride)
    got, counters = LC.device_layer(ctx, sc, depth, zeros.clone(), stride=stride, alias=True)
    check(LC.to_host(got), counters, layers[0], W, "aliased", pad_prim=0)
    # depth aliased only: prim_in NULL, prim_out separate
    depth = LC.device_depth0(ctx, sc, stride)
    planes = torch.full((14, H, stride), float(C.SENTINEL), dtype=torch.float32, device="cuda")
    ids = torch.full((H, stride), C.SENTINEL_ID, dtype=torch.int16, device="cuda")
    _, prim = ctx.rasterize_layer(sc.draws, sc.view, depth, None, 0, out=(Attributes(planes, ids, width=W), depth))
    torch.cuda.synchronize()
    check(LC.to_host((planes, ids, depth, prim)), None, layers[0], W, "depth aliased",
          outside=(np.full((H, stride), C.SENTINEL, np.float32), prim.cpu().numpy().view(np.uint32)))


@pytest.mark.parametrize("name,frame", [("intersecting", "70x37"), ("clipped_pane", "256x64")])
def test_row_bands_equal_the_full_frame(ctx, name, frame):
    """Uneven bands through offset pointers, peeled band by band, equal the same rows of the full frame's layers;
    other rows keep the sentinel. A band's counters equal the restatement's for that band."""
    W, H = LC.FRAMES[frame]
    sc, d0, layers = expected(name, frame)
    ctx.set_meshes(sc.meshes)
    for r0, r1 in ((0, 5), (5, 6), (6, H - 9), (H - 9, H)):
        depth, prim = LC.padded(d0, W + 1, C.SENTINEL), None
        hd, hp = d0[r0:r1], None
        for k, want in enumerate(layers):
            got, counters = LC.device_layer(ctx, sc, depth, prim, rows=(r0, r1))
            check(LC.to_host(got), None, want, W, f"{name} {frame} rows {r0}:{r1} layer {k}", rows=(r0, r1))
            b = LR.rasterize_layer(sc.meshes, sc.draws, sc.view.rows(r0, r1), hd, hp, sc.clip_near)
            assert counters[:3] == (b.stats, b.clip, b.layer), (r0, r1, k)
            depth, prim, hd, hp = got[2], got[3], b.depth, b.prim


def test_old_calls_are_undisturbed_by_layer_calls(ctx):
    """A pbr_rasterize_flags call after layer calls equals the same call before them, in every plane and counter, and
    reports a zero layer counter; the layer counter is zero before any layer call on the stream too."""
    W, H = LC.FRAMES["70x37"]
    sc, d0, layers = expected("clipped_pane", "70x37")
    flags = N.PBR_RASTER_CLIP_NEAR
    before = CC.device_rasterize(ctx, sc.meshes, sc.draws, sc.view, flags=flags)
    assert ctx.raster_layer_stats() == ZERO_LAYER
    depth = LC.device_depth0(ctx, sc, W + 1)
    got, counters = LC.device_layer(ctx, sc, depth, None)
    assert counters[2]["layer_fragments"] == layers[0].layer["layer_fragments"] > 0
    LC.device_layer(ctx, sc, got[2], got[3])
    after = CC.device_rasterize(ctx, sc.meshes, sc.draws, sc.view, flags=flags)
    assert ctx.raster_layer_stats() == ZERO_LAYER
    for b, a in zip(before[:3], after[:3]):
        assert O.bit_equal(b, a).all() if b.dtype == np.float32 else np.array_equal(b, a)
    assert before[3] == after[3] and before[4] == after[4]
    want = AR.rasterize(sc.meshes, sc.draws, sc.view, [], [], True, alpha_test=False)
    assert O.bit_equal(after[0][:, :, :W], want[0]).all() and after[3] == want[3] and after[4] == want[4]


def test_two_streams_with_layer_and_plain_calls_interleaved(gpu):
    """Layer calls and unflagged calls queued alternately on two streams (each stream has its own scratch and
    counters): every result is its own call's, and each stream's counters are those of its last call."""
    W, H = LC.FRAMES["256x64"]
    sc, d0, layers = expected("nested_far_near", "256x64")
    plain = AR.rasterize(sc.meshes, sc.draws, sc.view, [], [], alpha_test=False)
    with ShadingContext(0) as ctx:
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        ctx.set_meshes(sc.meshes)
        d_in = [LC.padded(l, W, 0) for l in (d0, layers[0].depth)]
        p_in = [None, LC.padded(layers[0].prim, W, 0)]
        torch.cuda.synchronize()
        outs = []
        for k in range(12):
            stream = (s1, s2)[k % 2]
            if k % 4 in (0, 3):  # s1: layer, plain, layer, plain ...; s2: plain, layer, plain, layer ...
                j = (k // 4) % 2  # layer 0 and layer 1 in turn
                at, prim = ctx.rasterize_layer(sc.draws, sc.view, d_in[j], p_in[j], stream=stream)
                outs.append((layers[j], at, prim))
            else:
                outs.append((None, ctx.rasterize(sc.draws, sc.view, stream=stream), None))
        # the last call on s1 (k = 10) was plain, on s2 (k = 11) a layer
        assert ctx.raster_stats(s1) == plain[3] and ctx.raster_layer_stats(s1) == ZERO_LAYER
        assert ctx.raster_layer_stats(s2) == outs[11][0].layer and ctx.raster_stats(s2) == outs[11][0].stats
        torch.cuda.synchronize()
        for k, (want, at, prim) in enumerate(outs):
            e = (plain[0], plain[1], plain[2]) if want is None else (want.planes, want.material, want.depth)
            assert O.bit_equal(at.planes.cpu().numpy(), e[0]).all(), k
            assert np.array_equal(at.material.cpu().numpy().view(np.uint16), e[1]), k
            assert O.bit_equal(at.depth.cpu().numpy(), e[2]).all(), k
            if want is not None:
                assert np.array_equal(prim.cpu().numpy().view(np.uint32), want.prim), k


def test_error_paths(gpu):
    """PBR_RASTER_ALPHA_TEST, unknown bits and bit 1, a null depth_in, prim_out or targets->depth, a null layer:
    PBR_ERR_INVALID_ARGUMENT, and the context is usable afterwards."""
    import ctypes

    W, H = LC.FRAMES["70x37"]
    sc, d0, layers = expected("nested_far_near", "70x37")
    with ShadingContext(0) as fresh:
        fresh.set_meshes(sc.meshes)
        depth = LC.padded(d0, W, 0)
        for bad in (N.PBR_RASTER_ALPHA_TEST, N.PBR_RASTER_ALPHA_TEST | N.PBR_RASTER_CLIP_NEAR, 2, 8):
            with pytest.raises(N.PbrError) as e:
                fresh.rasterize_layer(sc.draws, sc.view, depth, flags=bad)
            assert e.value.status == N.PBR_ERR_INVALID_ARGUMENT, bad
        planes = torch.empty((14, H, W), dtype=torch.float32, device=gpu)
        ids = torch.empty((H, W), dtype=torch.int16, device=gpu)
        prim = torch.empty((H, W), dtype=torch.int32, device=gpu)
        out = torch.empty((H, W), dtype=torch.float32, device=gpu)

        def layer(depth_in, prim_out):
            l = N.RasterLayer()
            l.depth_in, l.prim_in, l.prim_out = depth_in, None, prim_out
            return l

        for l, target in ((layer(None, prim.data_ptr()), (Attributes(planes, ids), out)),
                          (layer(depth.data_ptr(), None), (Attributes(planes, ids), out)),
                          (layer(depth.data_ptr(), prim.data_ptr()), Attributes(planes, ids)),  # targets->depth NULL
                          (layer(depth.data_ptr() + 2, prim.data_ptr()), (Attributes(planes, ids), out))):
            with pytest.raises(N.PbrError) as e:
                fresh._rasterize(sc.draws, sc.view, 0, target, None, layer=l)
            assert e.value.status == N.PBR_ERR_INVALID_ARGUMENT
        v, t = sc.view.to_c(), N.RasterTargets()
        assert fresh.lib.pbr_rasterize_layer(fresh.handle, None, 0, ctypes.byref(v), ctypes.byref(t), 0, None,
                                             None) == N.PBR_ERR_INVALID_ARGUMENT
        assert fresh.raster_layer_stats() == ZERO_LAYER  # the stream has not rasterised
        got, counters = LC.device_layer(fresh, sc, LC.padded(d0, W + 1, C.SENTINEL), None)
        check(LC.to_host(got), counters, layers[0], W, "after the refusals")


def test_bounds_checked_build_is_clean_and_equal(tmp_path, gpu):
    """raster_layer_cases.BOUNDS_CASES peeled under _lib/debug_bounds/libpbrshade.so in a fresh child process
    (PBR_LIB_PATH), which first checks which library it loaded: every layer equals the restatement and no index class
    is flagged (the reads of depth_in and of the floor plane are class "raster")."""
    import bounds_cases

    if not os.path.exists(C.DEBUG_LIB):
        pytest.fail(f"{C.DEBUG_LIB} missing: run `make -C physically_based_renderer_amd/csrc debug-bounds` first")
    problems = bounds_cases.debug_library_problems(bounds_cases.library_build_info(C.DEBUG_LIB), N.kernel_sources_sha())
    assert not problems, f"{C.DEBUG_LIB} is not the bounds-checked build of this checkout: " + "; ".join(problems)
    out = tmp_path / "raster_layer_dbg.npz"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "raster_layer_cases.py"), str(out)],
                       env={**os.environ, "PBR_LIB_PATH": C.DEBUG_LIB}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)  # numeric and unicode arrays only: allow_pickle stays False
    assert str(z["flavor"]) == "debug_bounds" and str(z["sources_sha"]) == N.kernel_sources_sha()
    assert (z["bounds"] < 0).all(), f"bounds violations (gbuffer/output/coverage/texel/light/lds/raster/mesh): {z['bounds']}"
    for name, frame in LC.BOUNDS_CASES:
        key = f"{name}_{frame}"
        sc, d0, layers = expected(name, frame)
        assert int(z[key + "__layers"]) == len(layers)
        for k, want in enumerate(layers):
            c = z[f"{key}__{k}__stats"].tolist()
            counters = (dict(zip(sorted(want.stats), c[:6])), dict(zip(sorted(want.clip), c[6:8])),
                        dict(zip(sorted(want.layer), c[8:])), ZERO_ALPHA)
            got = tuple(z[f"{key}__{k}__{p}"] for p in ("planes", "ids", "depth", "prim"))
            check(got, counters, want, LC.FRAMES[frame][0], f"debug-bounds {key} layer {k}")


# ---- End to end: the transparent pass over an opaque frame ----------------------------------------------------------

def glass_scene(W, H):
    """An opaque floor and sphere, then three transparent draws: a far pane, a near pane and a sphere in front of
    both, opacities 0.25, 0.5 and 0.8. The camera looks down +z from z = -2; the floor runs under the eye."""
    view = CC.camera(W, H)

    def pane(x0, x1, y0, y1, z, seed):
        m = CC.soup([(x0, y0, z), (x0, y1, z), (x1, y1, z), (x0, y0, z), (x1, y1, z), (x1, y0, z)], seed)
        m.vertices[:, 3:6] = (0.0, 0.0, -1.0)
        m.vertices[:, 6:9] = (1.0, 0.0, 0.0)
        m.vertices[:, 9:12] = (0.0, 1.0, 0.0)
        return m

    def placed(r, x, y, z):
        m = np.diag([r, r, r, 1.0]).astype(np.float32)
        m[3, 0:3] = (x, y, z)
        return tuple(m.ravel().tolist())

    meshes = [CC.floor(3, 4), S.uv_sphere(16, 8), pane(-1.5, 1.5, -0.8, 0.9, 2.0, 201),
              pane(-0.8, 1.2, -0.6, 0.7, 1.0, 202)]
    opaque = [Draw(mesh=0, material=0), Draw(mesh=1, material=1, world=placed(0.6, -0.5, -0.3, 1.5))]
    draws = [Draw(mesh=2, material=2, cull=1), Draw(mesh=3, material=3, cull=1),
             Draw(mesh=1, material=4, cull=0, world=placed(0.4, 0.2, 0.0, 0.0))]
    mats = [Material(diffuse_albedo=(0.6, 0.5, 0.4), roughness=0.8),
            Material(diffuse_albedo=(0.95, 0.64, 0.54), metallic=1.0, roughness=0.35),
            Material(diffuse_albedo=(0.2, 0.5, 0.9), roughness=0.3, opacity=0.25),
            Material(diffuse_albedo=(0.9, 0.3, 0.2), roughness=0.5, opacity=0.5),
            Material(diffuse_albedo=(0.3, 0.8, 0.4), roughness=0.2, opacity=0.8)]
    return LC.Scene(meshes, opaque, draws, view, True), mats


def test_draw_transparent_equals_the_composite_of_the_oracle(gpu):
    """Opaque rasterize -> resolve -> shade_frame (sky on the background), then draw_transparent. Target: the oracle's
    shading of each restated layer's resolved G-buffer, blended in layer order (tests/blend_layer_reference.py) over the
    oracle's opaque frame. Exact mode: bit-identical in RGBA32F, and the RGBA8 bytes identical; faithful mode: within
    1e-5 + L * 2^-22 relative per channel, L the layer count (the layers' own 1e-5, plus three roundings per blend of
    non-negative terms). The helper reports the chain's 3 layers and that it stopped on an empty one; the depth
    plane ends as the sequential pass's depth buffer."""
    W, H = LC.FRAMES["256x64"]
    sc, mats = glass_scene(W, H)
    flags = N.PBR_RASTER_CLIP_NEAR
    o = AR.rasterize(sc.meshes, sc.opaque, sc.view, mats, [], True, alpha_test=False)
    d0 = o[2]
    layers = LR.peel(sc.meshes, sc.draws, sc.view, d0, True)
    prims, zs, final_depth = LR.emulate(sc.meshes, sc.draws, sc.view, d0, True)
    L = len(layers) - 1
    assert L == len(prims) == 3
    assert all({int(m) for m in np.unique(l.material)} - {R.NONE} for l in layers[:-1])
    cfg = S.REFERENCE_SCENE.with_size(W, H)
    pc = S.scene_pass(cfg)
    assert pc.num_dir_lights == 4
    pc.flags |= N.PBR_FLAG_F0_PLANE
    opass, lights = oracle_pass_from_constants(pc), pc.light_array()
    sky = envmap.procedural_sky_rgba16(128, 64)
    og = RR.resolve(o[0], o[1], mats, [], RR.POINT)
    ref32 = O.shade_frame(list(og[0]), opass, lights, None, sky, og[2], O.OUTPUT_RGBA32F, n_threads=8)
    ref8 = O.shade_frame(list(og[0]), opass, lights, None, sky, og[2], O.OUTPUT_RGBA8, n_threads=8)
    seen = set()
    for l in layers[:-1]:
        g = RR.resolve(l.planes, l.material, mats, [], RR.POINT)
        assert np.array_equal(g[2] != 0, l.material != R.NONE)
        seen |= set(np.unique(g[1][g[2] != 0]).tolist())
        shaded = O.shade(list(g[0]), opass, lights, None, n_threads=8)
        ref32 = BR.blend(shaded, g[1], g[2], ref32)
        ref8 = BR.blend(shaded, g[1], g[2], ref8)
    assert seen == {np.float32(0.25), np.float32(0.5), np.float32(0.8)}

    with ShadingContext(0) as ctx:
        ctx.set_meshes(sc.meshes)
        ctx.set_materials(mats, [])
        ctx.set_sky_map(sky)

        def render(fmt, faithful=False):
            pc.flags = (pc.flags | N.PBR_FLAG_FAITHFUL) if faithful else (pc.flags & ~N.PBR_FLAG_FAITHFUL)
            ctx.set_pass(pc)
            at = ctx.rasterize(sc.opaque, sc.view, clip_near=True)
            gb, cov = ctx.resolve(at, RR.POINT)
            frame = ctx.shade_frame(gb, coverage=cov, fmt=fmt)
            done = ctx.draw_transparent(sc.draws, sc.view, at.depth, frame, flags=flags, filter=RR.POINT)
            torch.cuda.synchronize()
            pc.flags &= ~N.PBR_FLAG_FAITHFUL
            return frame.cpu().numpy(), at.depth.cpu().numpy(), done

        frame, depth, done = render(N.PBR_OUTPUT_RGBA32F)
        assert done == (3, True)
        assert O.bit_equal(depth, final_depth).all()
        eq = O.bit_equal(frame, ref32)
        print(f"transparent pass, exact: bit-identical {eq.mean():.6f}")
        assert eq.all(), np.argwhere(~eq)[:4].tolist()
        assert not O.bit_equal(frame, O.shade_frame(list(og[0]), opass, lights, None, sky, og[2], O.OUTPUT_RGBA32F,
                                                    n_threads=8)).all()  # the layers changed the frame
        frame8, _, done = render(N.PBR_OUTPUT_RGBA8_UNORM)
        assert done == (3, True) and np.array_equal(frame8, ref8), np.argwhere(frame8 != ref8)[:4].tolist()
        faithful, _, done = render(N.PBR_OUTPUT_RGBA32F, faithful=True)
        assert done == (3, True)
        err = O.rel_err(faithful, ref32).max()
        print(f"transparent pass, faithful: max_rel {err:.3g} (bound {1e-5 + L * 2.0 ** -22:.3g})")
        assert err <= 1e-5 + L * 2.0 ** -22
        # max_layers below the chain: the helper stops there and says that layers may remain
        ctx.set_pass(pc)
        at = ctx.rasterize(sc.opaque, sc.view, clip_near=True)
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device=gpu)
        assert ctx.draw_transparent(sc.draws, sc.view, at.depth, frame, flags=flags, max_layers=2) == (2, False)
        torch.cuda.synchronize()
        assert O.bit_equal(at.depth.cpu().numpy(), layers[1].depth).all()
