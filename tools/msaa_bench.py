"""Time four samples per pixel on the reference's 58 spheres (64 x 32 UV spheres, the overview
camera) at 1920x1080, in one process on one GPU, beside the one-sample sequence of the same library:

  1x      rasterize -> resolve -> shade_frame, stage by stage and whole;
  msaa    msaa_rasterize, msaa_fragments (per slot), resolve, shade_frame, msaa_resolve, stage by stage, and
          ShadingContext.draw_msaa whole (which also reads the slot counters once: one stream synchronisation).

HIP events, median of --steps calls after a clock ramp (tools/raster_bench.py's protocol); the library must be the
product build of this checkout. One JSON line per leg.

    python tools/msaa_bench.py [--width 1920 --height 1080] [--steps 50] [--log FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from physically_based_renderer_amd import _native as N  # noqa: E402
from physically_based_renderer_amd import envmap  # noqa: E402
from physically_based_renderer_amd import scenes as S  # noqa: E402
from physically_based_renderer_amd.renderer import Attributes, GBuffer, ShadingContext  # noqa: E402
from raster_bench import event_ms  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--slices", type=int, default=64)
    p.add_argument("--stacks", type=int, default=32)
    p.add_argument("--log")
    a = p.parse_args()
    W, H = a.width, a.height
    info = N.build_info()
    problems = N.build_problems(info)
    if problems:
        sys.exit("msaa_bench: not the product build of this checkout: " + "; ".join(problems))
    dev = torch.device("cuda", 0)
    lines = []

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        lines.append(line)

    emit({"tool": "msaa_bench", "width": W, "height": H, "sources_sha": info["sources_sha"],
          "device": torch.cuda.get_device_name(0), "steps": a.steps})
    cfg = S.REFERENCE_SCENE.with_size(W, H).with_camera(*S.OVERVIEW_CAMERA)
    meshes, draws = S.reference_scene_draws(a.slices, a.stacks)
    view = S.reference_scene_view(cfg)
    mats, texs = S.scene_materials(cfg)
    pc = S.scene_pass(cfg)
    pc.flags |= N.PBR_FLAG_FAITHFUL
    attrs = Attributes(torch.empty((14, H, W), dtype=torch.float32, device=dev),
                       torch.empty((H, W), dtype=torch.int16, device=dev))
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    gb = GBuffer(torch.empty((N.NUM_PLANES, H, W), dtype=torch.float32, device=dev),
                 opacity=torch.empty((H, W), dtype=torch.float32, device=dev))
    cov = torch.empty((H, W), dtype=torch.uint8, device=dev)
    frame = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    surface = torch.empty((4, H, W), dtype=torch.int64, device=dev)
    owner = torch.empty((H, W), dtype=torch.uint8, device=dev)
    with ShadingContext(0) as ctx:
        ctx.set_meshes(meshes)
        ctx.set_materials(mats, texs)
        ctx.set_sky_map(envmap.procedural_sky_rgba16(128, 64))
        ctx.set_pass(pc)

        def leg(name, fn, **extra):
            r = event_ms(fn, a.steps)
            r.update(leg=name, **extra)
            emit(r)
            return r["median_ms"]

        def one_x():
            at = ctx.rasterize(draws, view, out=(attrs, depth))
            ctx.resolve(at, N.PBR_FILTER_LINEAR, out=(gb, cov))
            ctx.shade_frame(gb, frame, coverage=cov)

        leg("1x_rasterize", lambda: ctx.rasterize(draws, view, out=(attrs, depth)))
        stats1 = ctx.raster_stats()
        leg("1x_resolve_materials", lambda: ctx.resolve(attrs, N.PBR_FILTER_LINEAR, out=(gb, cov)))
        leg("1x_shade_frame", lambda: ctx.shade_frame(gb, frame, coverage=cov))
        whole1 = leg("1x_whole", one_x, fragments=stats1["fragments"])

        leg("msaa_rasterize", lambda: ctx.msaa_rasterize(draws, view, surface=surface))
        stats4 = ctx.raster_stats()
        ctx.msaa_fragments(draws, view, surface, 0, out=(attrs, depth), owner=owner)
        pixels = ctx.msaa_stats()["slot_pixels"]
        n = max(1, sum(1 for q in pixels if q > 0))
        shaded = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in range(n)]
        for k in range(n):
            leg("msaa_fragments", lambda: ctx.msaa_fragments(draws, view, surface, k, out=(attrs, depth), owner=owner),
                slot=k, slot_pixels=pixels[k])
            leg("msaa_resolve_materials", lambda: ctx.resolve(attrs, N.PBR_FILTER_LINEAR, out=(gb, cov)), slot=k)
            leg("msaa_shade_frame", lambda: ctx.shade_frame(gb, shaded[k], coverage=cov), slot=k)
        leg("msaa_resolve", lambda: ctx.msaa_resolve(shaded, owner, out=frame), n_slots=n)
        done = []
        whole4 = leg("draw_msaa_whole", lambda: done.append(ctx.draw_msaa(draws, view, filter=N.PBR_FILTER_LINEAR, out=frame)[1]),
                     fragments=stats4["fragments"], slot_pixels=pixels)
        emit({"leg": "summary", "slots": done[-1], "draw_msaa_over_1x": whole4 / whole1})
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
