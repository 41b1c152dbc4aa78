"""Time the device rasteriser (pbr_rasterize) at 3840x2160 on three scenes, in one process on one GPU:

  reference    the reference's 58 spheres as 64 x 32 UV spheres (3,968 triangles each, 230,144 in all) from the
               overview camera;
  stress       ~10^6 triangles of about a pixel, uniformly over the frame;
  walkthrough  the reference scene over a floor of 64 x 64 quads, the eye one unit above the floor between the spheres
               of the bottom row: spheres and floor cross the near plane. Only near-plane clipping
               (pbr_rasterize_flags with PBR_RASTER_CLIP_NEAR) draws those triangles;
  cutout       the reference scene with all 58 spheres under one alpha-tested material whose opacity map is a
               256 x 256 checker with noise (libraries with PBR_RASTER_ALPHA_TEST only);
  glass        the reference scene plus four full-frame panes at decreasing depth in front of it, submitted far to
               near: four layers of the transparent pass (libraries with pbr_rasterize_layer only; its legs are below).

Four legs per scene:
  (a) the stages of one call, HIP events between them (pbr_debug_rasterize_timed): clears and table upload, the
      vertex transform, the setup kernel (with the small triangles' coverage), the large triangles' coverage, the
      per-pixel resolve; median of --steps calls after a clock ramp;
  (b) the whole call, events around ShadingContext.rasterize;
  (c) a device-to-device copy of the bytes the resolve stage writes (14 planes + the id: 58 B per pixel): the
      streaming yardstick;
  (d) reference scene only: the host route to the same planes, pbr_attributes_fill on 16 threads plus the upload
      (the analytic spheres, not the facets: DESIGN.md §12).
Legs (a) and (b) are taken unflagged and then, when the library has pbr_rasterize_flags, with PBR_RASTER_CLIP_NEAR
("clip": true in the line), with the clip counters of the call; and, when it has PBR_RASTER_ALPHA_TEST, with that flag
("alpha": true) and the alpha counters: on the first three scenes under a table without a tested material (the cost
of asking), on cutout against the same scene unflagged (the cost of the test).

The glass scene's legs:
  (e) the stages of one pbr_rasterize_layer call on the four panes (the first layer, over the opaque scene's depth)
      beside the stages of the unflagged call on the same draws;
  (f) pbr_blend_layer of a full frame (RGBA32F and RGBA8) beside a device-to-device copy that moves the same number
      of bytes (the blend reads 37 and writes 16 bytes per RGBA32F pixel: a copy of 26.5 B per pixel);
  (g) ShadingContext.draw_transparent whole -- four layers, each a rasterisation, a resolve, a shading pass over the
      whole frame and a blend, plus the empty fifth rasterisation that ends the loop -- beside the opaque frame
      (rasterize, resolve, shade_frame).

    python tools/raster_bench.py [--width 3840 --height 2160] [--steps 50] [--log profiles/r11/raster_bench.log]

--other-sources accepts a product build of another checkout (an A/B against the parent's library through
PBR_LIB_PATH); the line records whose sources it was built from.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physically_based_renderer_amd import _native as N  # noqa: E402
from physically_based_renderer_amd import scenes as S  # noqa: E402
from physically_based_renderer_amd.renderer import Attributes, Draw, Material, Mesh, ShadingContext, View  # noqa: E402

STAGES = ("clear_upload", "vertex", "setup_small", "large", "resolve")
BYTES_WRITTEN = 14 * 4 + 2


def event_ms(fn, steps, ramp_s=0.2):
    """Median / min / max of `steps` event-bracketed calls after a clock ramp of back-to-back calls."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < ramp_s:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def stress_scene(W, H, n_tris, seed=7):
    """n_tris triangles with vertices within ~0.9 pixel of a random centre, w in [0.5, 2], no culling."""
    rng = np.random.default_rng(seed)
    c = rng.uniform((0, 0), (W, H), (n_tris, 1, 2))
    p = c + rng.uniform(-0.9, 0.9, (n_tris, 3, 2))
    w = rng.uniform(0.5, 2.0, (n_tris, 3))
    v = np.zeros((n_tris, 3, 14), np.float32)
    v[..., 0] = (p[..., 0] / W * 2.0 - 1.0) * w
    v[..., 1] = (1.0 - p[..., 1] / H * 2.0) * w
    v[..., 2] = w
    v[..., 3:] = rng.normal(size=(n_tris, 3, 11)).astype(np.float32)
    near, far = 0.1, 100.0
    vp = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, far / (far - near), 1], [0, 0, -near * far / (far - near), 0]],
                  np.float32)
    view = View(view_proj=tuple(vp.ravel().tolist()), width=W, height=H)
    return [Mesh(v.reshape(-1, 14), np.arange(3 * n_tris, dtype=np.uint32))], [Draw(cull=1)], view


def walkthrough_scene(W, H, slices, stacks, quads=64):
    """The reference scene's draws plus a floor of quads x quads quads at y = -16.5 (half a unit under the bottom row
    of spheres), and a camera one unit above the floor between two spheres of that row, looking up the grid."""
    meshes, draws = S.reference_scene_draws(slices, stacks)
    j, i = np.meshgrid(np.arange(quads + 1), np.arange(quads + 1), indexing="ij")
    v = np.zeros(((quads + 1) ** 2, 14), np.float32)
    v[:, 0], v[:, 1], v[:, 2] = (-12.0 + 24.0 * i / quads).ravel(), -16.5, (-12.0 + 24.0 * j / quads).ravel()
    v[:, 4], v[:, 6], v[:, 11] = 1.0, 1.0, 1.0
    v[:, 12], v[:, 13] = (i / quads).ravel(), (j / quads).ravel()
    ring = quads + 1
    c, r = np.meshgrid(np.arange(quads), np.arange(quads))
    v00 = (r * ring + c).ravel()
    tris = np.stack([v00, v00 + ring, v00 + 1, v00 + 1, v00 + ring, v00 + ring + 1], -1)  # facing up
    meshes = meshes + [Mesh(v, tris.astype(np.uint32).reshape(-1))]
    draws = draws + [Draw(mesh=1, material=0)]
    view = S.look_at_view((1.25, -15.5, -0.5), (-7.5, -14.5, 1.5), float(np.pi / 3), W, H)
    return meshes, draws, view


def cutout_materials(n, seed=12):
    """n alpha-tested materials over one 256 x 256 opacity map: a checker of 16-texel squares (0 / 255) with noise:
    a fifth of the texels random bytes."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    tex = np.where(((i // 16 + j // 16) % 2) == 0, 255, 0)
    tex = np.where(rng.random((256, 256)) < 0.2, rng.integers(0, 256, (256, 256)), tex).astype(np.uint8)
    return [Material(flags=N.PBR_MAT_ALPHA_TEST, tex=(-1, -1, -1, -1, -1, 0)) for _ in range(n)], [tex]


def glass_panes(n=4):
    """n panes of 60 x 40 units around the overview camera's axis at z = -3, -5, ... (the camera is at z = -30, the
    spheres around z = 0): each covers the whole frame; far to near in submission order."""
    v = np.zeros((4, 14), np.float32)
    v[:, 0], v[:, 1] = (-30.0, 30.0, 30.0, -30.0), (13.0, 13.0, -27.0, -27.0)
    v[:, 5], v[:, 6], v[:, 10] = -1.0, 1.0, -1.0
    v[:, 12], v[:, 13] = (0.0, 1.0, 1.0, 0.0), (0.0, 0.0, 1.0, 1.0)
    mesh = Mesh(v, np.array([0, 1, 2, 0, 2, 3], np.uint32))
    return mesh, [(-3.0 - 2.0 * k) for k in range(n)]


def timed_layer_stages(ctx, draws, view, attrs, depth, depth_in, prim_out, steps):
    """timed_stages for pbr_rasterize_layer (pbr_debug_rasterize_layer_timed): the first layer, prim_in NULL."""
    timed = ctx.lib.pbr_debug_rasterize_layer_timed
    timed.argtypes = [ctypes.c_void_p, ctypes.POINTER(N.DrawDesc), ctypes.c_int32, ctypes.POINTER(N.RasterView),
                      ctypes.POINTER(N.RasterTargets), ctypes.c_uint32, ctypes.POINTER(N.RasterLayer), ctypes.c_void_p,
                      ctypes.POINTER(ctypes.c_float)]
    timed.restype = ctypes.c_int
    v = view.to_c()
    t = N.RasterTargets()
    ps = attrs.planes.stride(0) * 4
    t.planes[:] = [attrs.planes.data_ptr() + i * ps for i in range(14)]
    t.material, t.depth, t.row_stride = attrs.material.data_ptr(), depth.data_ptr(), int(attrs.row_stride)
    layer = N.RasterLayer()
    layer.depth_in, layer.prim_in, layer.prim_out = depth_in.data_ptr(), None, prim_out.data_ptr()
    c_draws = (N.DrawDesc * len(draws))(*[d.to_c(ctx.meshes) for d in draws])
    stream = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    ms = (ctypes.c_float * 5)()
    rows = []
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.2:  # clock ramp
        ctx.rasterize_layer(draws, view, depth_in, None, out=(attrs, depth), prim_out=prim_out)
    for _ in range(steps):
        N.check(timed(ctx.handle, c_draws, len(draws), ctypes.byref(v), ctypes.byref(t), 0, ctypes.byref(layer), stream,
                      ms), "pbr_debug_rasterize_layer_timed", ctx.handle)
        rows.append(list(ms))
    med = np.median(np.array(rows), axis=0)
    return {k: float(x) for k, x in zip(STAGES, med)}


def glass_legs(ctx, emit, cfg, ref_meshes, ref_draws, attrs, depth, steps):
    """Legs (e), (f) and (g) of the glass scene."""
    from physically_based_renderer_amd import envmap

    W, H = cfg.width, cfg.height
    dev = attrs.planes.device
    view = S.reference_scene_view(cfg)
    pane, zs = glass_panes()
    n_opaque = len(ref_draws)
    panes = [Draw(mesh=1, material=n_opaque + k, cull=1, world=S.translation(0.0, 0.0, z)) for k, z in enumerate(zs)]
    ctx.set_meshes(ref_meshes + [pane])
    ctx.set_materials([Material()] * n_opaque + [Material(diffuse_albedo=(0.3 + 0.2 * k, 0.6, 0.9 - 0.2 * k),
                                                         roughness=0.4, opacity=0.2 + 0.1 * k) for k in range(len(zs))])
    ctx.set_sky_map(envmap.procedural_sky_rgba16(128, 64))
    pc = S.scene_pass(cfg)
    pc.flags |= N.PBR_FLAG_F0_PLANE | N.PBR_FLAG_FAITHFUL
    ctx.set_pass(pc)
    ctx.rasterize(ref_draws, view, out=(attrs, depth))
    depth0 = depth.clone()
    prim = torch.empty((H, W), dtype=torch.int32, device=dev)
    # (e) one layer call beside the unflagged call, both on the four panes
    ctx.rasterize_layer(panes, view, depth0, None, out=(attrs, depth), prim_out=prim)
    stats = ctx.raster_stats()
    stats.update(ctx.raster_layer_stats())
    emit({"scene": "glass", "leg": "e_layer_call", "stats": stats, "draws": len(panes),
          "covered_pixels": int((attrs.material != -1).sum().item())})
    for layer in (False, True):
        st = (timed_layer_stages(ctx, panes, view, attrs, depth, depth0, prim, steps) if layer
              else timed_stages(ctx, panes, view, attrs, depth, steps))
        st.update(leg="e_stages_ms", scene="glass", layer=layer, coverage_ms=st["setup_small"] + st["large"])
        emit(st)
        fn = ((lambda: ctx.rasterize_layer(panes, view, depth0, None, out=(attrs, depth), prim_out=prim)) if layer
              else (lambda: ctx.rasterize(panes, view, out=(attrs, depth))))
        whole = event_ms(fn, steps)
        whole.update(leg="e_whole_call", scene="glass", layer=layer)
        emit(whole)
    # (f) the blend beside a copy that moves as many bytes
    ctx.rasterize_layer(panes, view, depth0, None, out=(attrs, depth), prim_out=prim)
    gb, cov = ctx.resolve(attrs)
    shaded = ctx.shade(gb)
    for fmt, dtype, moved in (("rgba32f", torch.float32, 16 + 4 + 1 + 16 + 16), ("rgba8", torch.uint8, 16 + 4 + 1 + 4 + 4)):
        frame = torch.zeros((H, W, 4), dtype=dtype, device=dev)
        b = event_ms(lambda: ctx.blend_layer(shaded, gb.opacity, cov, frame), steps)
        half = torch.empty(W * H * moved // 2, dtype=torch.uint8, device=dev)
        other = torch.empty_like(half)
        c = event_ms(lambda: other.copy_(half), steps)
        b.update(leg="f_blend_layer", scene="glass", format=fmt, bytes_moved_per_pixel=moved,
                 copy_same_bytes_median_ms=c["median_ms"], blend_over_copy=b["median_ms"] / c["median_ms"],
                 covered_pixels=int((cov != 0).sum().item()))
        emit(b)
    # (g) the whole transparent pass beside the opaque frame
    frame = torch.empty((H, W, 4), dtype=torch.float32, device=dev)

    def opaque_frame():
        at = ctx.rasterize(ref_draws, view, out=(attrs, depth))
        ctx.resolve(at, out=(gb, cov))
        ctx.shade_frame(gb, frame, coverage=cov)

    done = []

    def transparent():
        depth.copy_(depth0)
        done.append(ctx.draw_transparent(panes, view, depth, frame))

    o = event_ms(opaque_frame, steps)
    o.update(leg="g_opaque_frame", scene="glass")
    emit(o)
    opaque_frame()
    t = event_ms(transparent, steps)
    t.update(leg="g_draw_transparent", scene="glass", layers=done[-1][0], stopped_on_empty=done[-1][1],
             per_layer_ms=t["median_ms"] / max(done[-1][0], 1), over_opaque_frame=t["median_ms"] / o["median_ms"])
    emit(t)


def timed_stages(ctx, draws, view, attrs, depth, steps, clip=False, alpha=False):
    """Per-stage medians of `steps` timed calls (each synchronises; the clock ramp is the untimed loop before)."""
    argtypes = [ctypes.c_void_p, ctypes.POINTER(N.DrawDesc), ctypes.c_int32, ctypes.POINTER(N.RasterView),
                ctypes.POINTER(N.RasterTargets), ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    kw = {**({"clip_near": True} if clip else {}), **({"alpha_test": True} if alpha else {})}
    if clip or alpha:
        timed = ctx.lib.pbr_debug_rasterize_flags_timed
        timed.argtypes = argtypes[:5] + [ctypes.c_uint32] + argtypes[5:]
        flags = (N.PBR_RASTER_CLIP_NEAR if clip else 0) | (N.PBR_RASTER_ALPHA_TEST if alpha else 0)

        def fn(h, c_draws, n, v, t, stream, ms):
            return timed(h, c_draws, n, v, t, flags, stream, ms)
    else:
        timed = fn = ctx.lib.pbr_debug_rasterize_timed
        timed.argtypes = argtypes
    timed.restype = ctypes.c_int
    v = view.to_c()
    t = N.RasterTargets()
    ps = attrs.planes.stride(0) * 4
    t.planes[:] = [attrs.planes.data_ptr() + i * ps for i in range(14)]
    t.material, t.depth, t.row_stride = attrs.material.data_ptr(), depth.data_ptr(), int(attrs.row_stride)
    c_draws = (N.DrawDesc * len(draws))(*[d.to_c(ctx.meshes) for d in draws])
    stream = ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))
    ms = (ctypes.c_float * 5)()
    rows = []
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.2:  # clock ramp
        ctx.rasterize(draws, view, out=(attrs, depth), **kw)
    for _ in range(steps):
        N.check(fn(ctx.handle, c_draws, len(draws), ctypes.byref(v), ctypes.byref(t), stream, ms),
                "pbr_debug_rasterize_timed", ctx.handle)
        rows.append(list(ms))
    med = np.median(np.array(rows), axis=0)
    return {k: float(x) for k, x in zip(STAGES, med)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--stress-triangles", type=int, default=1_000_000)
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--stacks", type=int, default=32)
    ap.add_argument("--log", default=None, help="append the result lines to this file too")
    ap.add_argument("--other-sources", action="store_true",
                    help="accept a product build of another checkout's sources (A/B through PBR_LIB_PATH)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("raster_bench: no GPU visible (timings are taken on the device only)")
    info = N.build_info()
    problems = N.build_problems(info, info["sources_sha"] if a.other_sources else None)
    if problems:
        sys.exit("raster_bench: not the product build of this checkout: " + "; ".join(problems))
    W, H = a.width, a.height
    dev = torch.device("cuda", 0)
    lines = []

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        lines.append(line)

    can_clip = hasattr(N.lib(), "pbr_rasterize_flags")
    can_alpha = hasattr(N.lib(), "pbr_last_raster_alpha_stats")
    can_layer = hasattr(N.lib(), "pbr_rasterize_layer")
    emit({"tool": "raster_bench", "width": W, "height": H, "sources_sha": info["sources_sha"],
          "checkout_sha": N.kernel_sources_sha(), "library": os.path.relpath(info["path"], ROOT),
          "has_rasterize_flags": can_clip, "has_alpha_test": can_alpha, "has_rasterize_layer": can_layer,
          "device": torch.cuda.get_device_name(0), "steps": a.steps, "resolve_bytes_per_pixel": BYTES_WRITTEN})
    cfg = S.REFERENCE_SCENE.with_size(W, H).with_camera(*S.OVERVIEW_CAMERA)
    ref_meshes, ref_draws = S.reference_scene_draws(a.slices, a.stacks)
    scenes = [("reference", ref_meshes, ref_draws, S.reference_scene_view(cfg)),
              ("stress",) + stress_scene(W, H, a.stress_triangles),
              ("walkthrough",) + walkthrough_scene(W, H, a.slices, a.stacks)]
    if can_alpha:
        scenes.append(("cutout", ref_meshes, ref_draws, S.reference_scene_view(cfg)))
    attrs = Attributes(torch.empty((14, H, W), dtype=torch.float32, device=dev),
                       torch.empty((H, W), dtype=torch.int16, device=dev))
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    src = torch.empty(W * H * BYTES_WRITTEN, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    with ShadingContext(0) as ctx:
        c = event_ms(lambda: dst.copy_(src), a.steps)
        c.update(leg="c_d2d_copy_58B_per_pixel", gb_per_s=2 * src.numel() / (c["median_ms"] * 1e-3) / 1e9)
        emit(c)
        for name, meshes, draws, view in scenes:
            ctx.set_meshes(meshes)
            if can_alpha:  # cutout: every sphere tested; the other scenes: a table without a tested material
                ctx.set_materials(*(cutout_materials(len(draws)) if name == "cutout" else ([Material()] * 64, [])))
            legs = [(False, False)] + ([(True, False)] if can_clip and name != "cutout" else [])
            legs += [(False, True)] if can_alpha else []
            for clip, alpha in legs:
                kw = {**({"clip_near": True} if clip else {}), **({"alpha_test": True} if alpha else {})}
                ctx.rasterize(draws, view, out=(attrs, depth), **kw)
                stats = ctx.raster_stats()
                if clip:
                    stats.update(ctx.raster_clip_stats())
                if alpha:
                    stats.update(ctx.raster_alpha_stats())
                covered = int((attrs.material != -1).sum().item())
                emit({"scene": name, "clip": clip, "alpha": alpha, "stats": stats, "covered_pixels": covered,
                      "vertices": int(sum(m.vertices.shape[0] for m in meshes)), "draws": len(draws)})
                st = timed_stages(ctx, draws, view, attrs, depth, a.steps, clip, alpha)
                st.update(leg="a_stages_ms", scene=name, clip=clip, alpha=alpha,
                          coverage_ms=st["setup_small"] + st["large"], resolve_over_copy=st["resolve"] / c["median_ms"])
                emit(st)
                whole = event_ms(lambda: ctx.rasterize(draws, view, out=(attrs, depth), **kw), a.steps)
                whole.update(leg="b_whole_call", scene=name, clip=clip, alpha=alpha)
                emit(whole)
        if can_layer:
            glass_legs(ctx, emit, cfg, ref_meshes, ref_draws, attrs, depth, a.steps)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            planes, mat = S.fill_attributes_host(cfg, n_threads=16)
            t1 = time.perf_counter()
            Attributes.from_host(planes, mat, dev)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0, t1 - t0))
        host.sort()
        emit({"leg": "d_host_attributes_fill_plus_upload", "scene": "reference (analytic spheres)",
              "median_ms": host[1][0] * 1e3, "fill_ms": host[1][1] * 1e3})
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
