"""The device rasteriser against the float64 geometric truth of tests/raster_truth.py ("Distance of the
rule set from exact geometry"): the planes pbr_rasterize, pbr_rasterize_flags and pbr_rasterize_layer write are held to
the truth directly, not through the numpy restatements -- these tests would mean the same if a restatement were
deleted. The scenes, frames, bounds, caps and counter intervals are those of tests/test_raster_truth_host.py, whose
docstring says what the truth abstains on; every call writes into canvases with the odd row stride W + 1.

One test per flavour of entry point, looping over its cases. Each prints one line per case and frame (checked pixels,
unsure pixels, the worst excess beyond the five-point interval in units of 2^-24 S_k; the bound is 32) and collects
every failure before it asserts, so that one run shows them all. Most of a test's time is the truth on the host."""
import pytest
import torch

import raster_alpha_cases as AC
import raster_cases as C
import raster_clip_cases as CC
import raster_layer_cases as LC
import raster_truth as RT
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd.renderer import ShadingContext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    c = ShadingContext(0)
    yield c
    c.close()


def padding_untouched(what, W, planes, ids, depth):
    ok = (planes[:, :, W:] == C.SENTINEL).all() and (ids[:, W:] == C.SENTINEL_ID).all() and \
        (depth[:, W:] == C.SENTINEL).all()
    return [] if ok else [f"{what}: the padding column was written"]


def flat_failures(ctx, family, name, frame):
    """One plain, clipped, alpha-tested or soup case on the device against its truth: the failure lines."""
    m, d, v, clip_near, mats, texs, _ = RT.scene(family, name, frame)
    T = RT.truth(family, name, frame)
    what = f"{family} {name} {frame}"
    clip = alpha = None
    if family == "alpha":
        planes, ids, depth, stats, clip, alpha = AC.device_rasterize(ctx, m, d, v, mats, texs, clip_near)
        clip = clip if clip_near else None
    elif clip_near:
        planes, ids, depth, stats, clip = CC.device_rasterize(ctx, m, d, v)
    else:
        planes, ids, depth, stats = C.device_rasterize(ctx, m, d, v)
    rep = T.check(T.winners(), planes, ids, depth, what=what)
    print(rep.line(what))
    fails = rep.failures + rep.caps(what) + RT.counter_failures(T, stats, clip, alpha, what)
    if T.marginal and (family, name) not in RT.MARGINAL_ALLOWED:
        fails.append(f"{what}: {T.marginal} triangles of marginal area")
    return fails + padding_untouched(what, v.width, planes, ids, depth)


def layer_failures(ctx, name, frame):
    """One layer case on the device: the opaque depth, then layer after layer until the device reports an empty one."""
    m, d, v, clip_near, _, _, opaque = RT.scene("layer", name, frame)
    sc = LC.Scene(m, opaque, d, v, clip_near)
    T = RT.truth("layer", name, frame)
    what = f"layer {name} {frame}"
    W = v.width
    fails, reps = [], []
    ctx.set_meshes(m)
    if opaque:  # the incoming depth is itself a rasterisation: held to the truth of the opaque draws
        flags = N.PBR_RASTER_CLIP_NEAR if clip_near else 0
        p0, i0, z0, s0, c0 = CC.device_rasterize(ctx, m, opaque, v, set_meshes=False, flags=flags)
        T0 = RT.Truth(m, opaque, v, clip_near)
        rep = T0.check(T0.winners(), p0, i0, z0, what=what + " opaque")
        fails += rep.failures + RT.counter_failures(T0, s0, c0 if clip_near else None, None, what + " opaque")
    depth, prim = LC.device_depth0(ctx, sc, W + 1), None
    torch.cuda.synchronize()
    prev = depth.cpu().numpy()[:, :W]
    sure, wins = T.layers(prev)
    for k in range(16):
        got, (stats, clip, layer, _) = LC.device_layer(ctx, sc, depth, prim)
        planes, ids, dep, pr = LC.to_host(got)
        rep = T.check(wins[min(k, len(wins) - 1)], planes, ids, dep, background_depth=prev, prim=pr,
                      what=f"{what} layer {k}")
        fails += rep.failures + RT.counter_failures(T, stats, clip if clip_near else None, None, f"{what} layer {k}")
        fails += padding_untouched(f"{what} layer {k}", W, planes, ids, dep)
        reps.append(rep)
        if layer["layer_fragments"] == 0:
            break
        depth, prim, prev = got[2], got[3], dep[:, :W]
    else:
        fails.append(f"{what}: no empty layer within 16")
    if len(wins) > len(reps):
        fails.append(f"{what}: {len(reps)} layers, the truth has {len(wins)}")
    fails += RT.sequence_caps(what, sure, reps)
    if T.marginal and ("layer", name) not in RT.MARGINAL_ALLOWED:
        fails.append(f"{what}: {T.marginal} triangles of marginal area")
    return fails


def test_plain_calls_inside_the_truth(ctx):
    """pbr_rasterize: the eight plain scenes in both frames and the three soups in 71x37 and 256x64."""
    fails = []
    for name in RT.PLAIN_CASES:
        for frame in RT.FRAMES:
            fails += flat_failures(ctx, "plain", name, frame)
    for seed in RT.SOUP_SEEDS:
        for frame in RT.SOUP_FRAMES:
            fails += flat_failures(ctx, "soup", str(seed), frame)
    assert not fails, "\n".join(fails)


def test_clip_near_calls_inside_the_truth(ctx):
    """pbr_rasterize_flags(PBR_RASTER_CLIP_NEAR): the five clip scenes and the 24 single triangles."""
    fails = []
    for name in RT.CLIP_CASES + CC.SINGLE_CASES:
        for frame in RT.FRAMES:
            fails += flat_failures(ctx, "clip", name, frame)
    assert not fails, "\n".join(fails)


def test_alpha_test_calls_inside_the_truth(ctx):
    """pbr_rasterize_flags(PBR_RASTER_ALPHA_TEST): the checker and wrap scenes."""
    fails = []
    for name in RT.ALPHA_CASES:
        for frame in RT.FRAMES:
            if not RT.scene("alpha", name, frame)[3]:
                fails += flat_failures(ctx, "alpha", name, frame)
    assert not fails, "\n".join(fails)


def test_clip_near_alpha_test_calls_inside_the_truth(ctx):
    """pbr_rasterize_flags with both flags: the clipped, alpha-tested floor and sphere."""
    fails, ran = [], 0
    for name in RT.ALPHA_CASES:
        for frame in RT.FRAMES:
            if RT.scene("alpha", name, frame)[3]:
                fails += flat_failures(ctx, "alpha", name, frame)
                ran += 1
    assert ran == 2
    assert not fails, "\n".join(fails)


def test_layer_sequences_inside_the_truth(ctx):
    """pbr_rasterize_layer, each case's sequence until the device reports an empty layer: every layer's winner,
    prim_out, planes and depth, and the depth passed through where a layer has no winner."""
    fails = []
    for name in RT.LAYER_CASES:
        for frame in RT.FRAMES:
            fails += layer_failures(ctx, name, frame)
    assert not fails, "\n".join(fails)
