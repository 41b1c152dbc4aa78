"""pbr_rasterize_flags with PBR_RASTER_CLIP_NEAR on the GPU (csrc/raster.h): triangles across the
near plane are cut and drawn. Every comparison is bit for bit (oracle.bit_equal, NaN patterns equal) against the numpy
restatement of tests/raster_clip_reference.py -- all 14 planes, the material plane, the depth plane -- and the eight
counters exactly. tests/test_raster_clip_host.py checks the restatement against the rules themselves. A library
without pbr_rasterize_flags fails every test here (the binding raises); none is skipped."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_cases as C
import raster_clip_cases as CC
import raster_clip_reference as CR
import raster_reference as R
import resolve_reference as RR
from conftest import ROOT, oracle_pass_from_constants
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import envmap
from physically_based_renderer_amd import scenes as S
from physically_based_renderer_amd.renderer import ShadingContext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    c = ShadingContext(0)
    yield c
    c.close()


_expected = {}


def expected(name, frame):
    """The flagged restatement of one case, computed once and shared."""
    if (name, frame) not in _expected:
        W, H = CC.FRAMES[frame]
        _expected[(name, frame)] = CR.rasterize(*CC.case(name, W, H))
    return _expected[(name, frame)]


def check(got, want, W, what, rows=None):
    planes, ids, depth, stats, clip = got
    eplanes, eids, edepth, estats, eclip = want
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
        assert clip == eclip, f"{what}: clip stats {clip} != {eclip}"
    # the padding columns of a strided canvas, and the rows outside a band, are never written
    assert (planes[:, :, W:] == C.SENTINEL).all() and (depth[:, W:] == C.SENTINEL).all()
    assert (ids[:, W:] == C.SENTINEL_ID).all()
    outside = np.ones(planes.shape[1], bool)
    outside[r0:r1] = False
    assert (planes[:, outside] == C.SENTINEL).all() and (depth[outside] == C.SENTINEL).all()
    assert (ids[outside] == C.SENTINEL_ID).all()


@pytest.mark.parametrize("frame", list(CC.FRAMES))
@pytest.mark.parametrize("name", CC.CASES)
def test_case_equals_the_restatement(ctx, name, frame):
    """Every case of raster_clip_cases.CASES in both frames, into an odd row stride (width + 1: the scalar stores) and
    into an even one (width: the paired stores)."""
    W, H = CC.FRAMES[frame]
    m, d, v = CC.case(name, W, H)
    want = expected(name, frame)
    print(name, frame, want[3], want[4])
    for stride in (W + 1, W):
        got = CC.device_rasterize(ctx, m, d, v, stride=stride)
        check(got, want, W, f"{name} {frame} stride {stride}")


@pytest.mark.parametrize("name,frame", [("floor_quad", "70x37"), ("inside_sphere", "256x64")])
def test_row_bands_equal_the_full_frame(ctx, name, frame):
    """Uneven bands through offset pointers equal the same rows of the full frame; other rows keep the sentinel."""
    W, H = CC.FRAMES[frame]
    m, d, v = CC.case(name, W, H)
    want = expected(name, frame)
    for r0, r1 in ((0, 5), (5, 6), (6, H - 9), (H - 9, H)):
        got = CC.device_rasterize(ctx, m, d, v, rows=(r0, r1))
        check(got, want, W, f"{name} {frame} rows {r0}:{r1}", rows=(r0, r1))
        band = CR.rasterize(m, d, v.rows(r0, r1))
        assert got[3] == band[3] and got[4] == band[4], (r0, r1)


def test_no_flags_is_pbr_rasterize_and_drops_the_floor(ctx):
    """flags = 0 through pbr_rasterize_flags equals pbr_rasterize bit for bit on case (a), with the same statistics
    and zero clip counters; and that result is today's: both triangles skipped near, the frame all background. An
    unknown flag bit is refused."""
    W, H = CC.FRAMES["70x37"]
    m, d, v = CC.case("floor_quad", W, H)
    old = CC.device_rasterize(ctx, m, d, v, flags=None)
    new = CC.device_rasterize(ctx, m, d, v, flags=0)
    want = R.rasterize(m, d, v)
    zeros = dict.fromkeys(CR.CLIP_STAT_NAMES, 0)
    for got in (old, new):
        check(got, want + (zeros,), W, "unflagged floor_quad")
    assert old[3]["skipped_near"] == new[3]["skipped_near"] == 2 and (new[1][:, :W] == R.NONE).all()
    for bad in (2, 3, 1 << 31):
        with pytest.raises(N.PbrError) as e:
            ctx.rasterize_flags(d, v, bad)
        assert e.value.status == N.PBR_ERR_INVALID_ARGUMENT, bad
    flagged = CC.device_rasterize(ctx, m, d, v)  # the context is usable after the refusals
    check(flagged, expected("floor_quad", "70x37"), W, "flagged floor_quad")
    assert (flagged[1][:, :W] == 1).mean() > 0.15


def test_two_streams_flagged_and_unflagged_interleaved(gpu):
    """Flagged and unflagged rasterisations queued alternately on two streams (each stream has its own scratch, laid
    out per call): every result is its own call's, and each stream's counters are its last call's."""
    W, H = CC.FRAMES["256x64"]
    m, d, v = CC.case("floor_sphere_floor", W, H)
    want_clip, want_plain = expected("floor_sphere_floor", "256x64"), R.rasterize(m, d, v)
    with ShadingContext(0) as ctx:
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        ctx.set_meshes(m)
        torch.cuda.synchronize()
        outs = []
        for k in range(8):
            clip = k % 4 in (0, 3)  # s1: clip, plain, clip, plain; s2: plain, clip, plain, clip
            outs.append((want_clip if clip else want_plain, ctx.rasterize(d, v, stream=(s1, s2)[k % 2], clip_near=clip)))
        # the last call on s1 (k = 6) was plain, on s2 (k = 7) flagged
        assert ctx.raster_stats(s1) == want_plain[3] and ctx.raster_clip_stats(s1) == {"clipped_near": 0, "clip_pieces": 0}
        assert ctx.raster_stats(s2) == want_clip[3] and ctx.raster_clip_stats(s2) == want_clip[4]
        torch.cuda.synchronize()
        for k, (want, at) in enumerate(outs):
            assert O.bit_equal(at.planes.cpu().numpy(), want[0]).all(), k
            assert np.array_equal(at.material.cpu().numpy().view(np.uint16), want[1]), k
            assert O.bit_equal(at.depth.cpu().numpy(), want[2]).all(), k


def test_bounds_checked_build_is_clean_and_equal(tmp_path, gpu):
    """raster_clip_cases.BOUNDS_CASES -- (a), (g), (i), flagged -- under _lib/debug_bounds/libpbrshade.so in a fresh
    child process (PBR_LIB_PATH), which first checks which library it loaded: the results equal the restatement and no
    index class is flagged (the PosH array and the two-slot large list are class "raster")."""
    import bounds_cases

    if not os.path.exists(C.DEBUG_LIB):
        pytest.fail(f"{C.DEBUG_LIB} missing: run `make -C physically_based_renderer_amd/csrc debug-bounds` first")
    problems = bounds_cases.debug_library_problems(bounds_cases.library_build_info(C.DEBUG_LIB), N.kernel_sources_sha())
    assert not problems, f"{C.DEBUG_LIB} is not the bounds-checked build of this checkout: " + "; ".join(problems)
    out = tmp_path / "raster_clip_dbg.npz"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "raster_clip_cases.py"), str(out)],
                       env={**os.environ, "PBR_LIB_PATH": C.DEBUG_LIB}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)  # numeric and unicode arrays only: allow_pickle stays False
    assert str(z["flavor"]) == "debug_bounds" and str(z["sources_sha"]) == N.kernel_sources_sha()
    assert (z["bounds"] < 0).all(), f"bounds violations (gbuffer/output/coverage/texel/light/lds/raster/mesh): {z['bounds']}"
    for name, frame in CC.BOUNDS_CASES:
        key = f"{name}_{frame}"
        want = expected(name, frame)
        counters = z[key + "__stats"].tolist()
        stats, clip = dict(zip(sorted(want[3]), counters[:6])), dict(zip(sorted(want[4]), counters[6:]))
        check((z[key + "__planes"], z[key + "__ids"], z[key + "__depth"], stats, clip), want, CC.FRAMES[frame][0],
              "debug-bounds " + key)


def test_clipped_rasterise_resolve_shade_equals_the_oracle(gpu):
    """End to end on case (h) at 256x64 under the reference scene's materials and four directional lights: flagged
    rasterize -> resolve -> shade_frame. The rasterised planes equal the restatement; the resolved G-buffer equals the
    resolve's restatement on them; the frame (exact mode, sky pass on the resolved coverage) equals the oracle's on
    those planes bit for bit, the faithful mode within 1e-5."""
    W, H = CC.FRAMES["256x64"]
    cfg = S.REFERENCE_SCENE.with_size(W, H)
    meshes, draws, view = CC.case("floor_sphere_floor", W, H)
    planes, ids, depth, stats, clip = expected("floor_sphere_floor", "256x64")
    assert clip["clipped_near"] > 0 and set(np.unique(ids).tolist()) == {0, 1, R.NONE}
    mats, texs = S.scene_materials(cfg)
    pc = S.scene_pass(cfg)
    assert pc.num_dir_lights == 4
    sky = envmap.procedural_sky_rgba16(128, 64)
    with ShadingContext(0) as ctx:
        ctx.set_meshes(meshes)
        ctx.set_materials(mats, texs)
        ctx.set_sky_map(sky)
        at = ctx.rasterize(draws, view, clip_near=True)
        assert ctx.raster_stats() == stats and ctx.raster_clip_stats() == clip
        torch.cuda.synchronize()
        assert O.bit_equal(at.planes.cpu().numpy(), planes).all()
        assert np.array_equal(at.material.cpu().numpy().view(np.uint16), ids)
        assert O.bit_equal(at.depth.cpu().numpy(), depth).all()
        rwant = RR.resolve(planes, ids, mats, texs, RR.LINEAR)
        gb, cov = ctx.resolve(at, RR.LINEAR)
        torch.cuda.synchronize()
        assert O.bit_equal(gb.planes.cpu().numpy(), rwant[0]).all()
        assert O.bit_equal(gb.opacity.cpu().numpy(), rwant[1]).all()
        assert np.array_equal(cov.cpu().numpy(), rwant[2]) and np.array_equal(rwant[2] != 0, ids != R.NONE)
        ctx.set_pass(pc)
        frame = ctx.shade_frame(gb, coverage=cov).cpu().numpy()
        ref = O.shade_frame(list(rwant[0]), oracle_pass_from_constants(pc), pc.light_array(), None, sky, rwant[2],
                            O.OUTPUT_RGBA32F, n_threads=8)
        print(f"clipped floor and sphere: bit-identical {O.bit_equal(frame, ref).mean():.6f}")
        assert O.bit_equal(frame, ref).all()
        pc.flags |= N.PBR_FLAG_FAITHFUL
        ctx.set_pass(pc)
        faithful = ctx.shade_frame(gb, coverage=cov).cpu().numpy()
        pc.flags &= ~N.PBR_FLAG_FAITHFUL
    err = O.rel_err(faithful, ref).max()
    print(f"faithful max_rel {err:.3g}")
    assert err <= 1e-5
