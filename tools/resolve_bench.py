"""Time the device material resolve (pbr_resolve_materials) on config 4 against the only other route
to the same device G-buffer and against the box's streaming rate, in one process on one GPU:

  (a) the resolve kernel, point and linear filter: ms per frame (HIP events, median) and achieved GB/s on its
      algorithmic bytes (14 attribute floats + a 2-byte id read, 15 planes + opacity + a coverage byte written:
      123 B per pixel; texel fetches are not counted);
  (b) the host route: pbr_gbuffer_fill on 16 threads + GBuffer.from_host (15 fp32 planes over PCIe), host clock
      around work that ends in a device synchronise;
  (c) a device-to-device copy moving (a)'s byte count (half read, half written): the streaming yardstick;
  (d) the trilinear resolve (pbr_resolve_materials_mip) beside (a)'s linear leg, the yardstick of this leg: (i) lod 0
      everywhere (a bias of -64 clamps every sample to level 0: the magnified case, one bilinear per sample), the
      scene's own footprints (bias 0), (ii) bias 1.5 (every sample between two levels: two bilinears); and
      pbr_generate_mips on the scene's textures (host clock: the call synchronises its stream);
  (e) the anisotropic resolve (pbr_resolve_materials_aniso), each leg beside the leg of (d) that samples as many
      levels, with that leg's own min / max over its median as the spread: max_anisotropy 1 (the trilinear fetches through
      the tap loop) under bias 0 and 1.5, max_anisotropy 8 on the scene's own footprints, and a worst case --
      the scene's attributes under a 10 : 1 UV ramp and bias 0.5, every sample 8 taps on two levels -- with its time
      per bilinear against (ii)'s.

    python tools/resolve_bench.py [--width 3840 --height 2160] [--steps 50] [--log profiles/r09/resolve_bench.log]

The resolved planes are checked bit for bit against the host fill's before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physically_based_renderer_amd import _native as N  # noqa: E402
from physically_based_renderer_amd import scenes as S  # noqa: E402
from physically_based_renderer_amd.renderer import GBuffer, ShadingContext  # noqa: E402

BYTES_READ = 14 * 4 + 2
BYTES_WRITTEN = 15 * 4 + 4 + 1


def event_ms(fn, steps, ramp_s=0.2):
    """Median / min / max of `steps` event-bracketed calls after a clock ramp of back-to-back calls."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < ramp_s:
        for _ in range(8):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--log", default=None, help="append the result lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resolve_bench: no GPU visible (timings are taken on the device only)")
    problems = N.build_problems()
    if problems:
        sys.exit("resolve_bench: not the product build of this checkout: " + "; ".join(problems))
    cfg = S.CONFIGS[4].with_size(a.width, a.height)
    dev = torch.device("cuda", 0)
    px = cfg.width * cfg.height
    total = px * (BYTES_READ + BYTES_WRITTEN)
    lines = []

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        lines.append(line)

    emit({"tool": "resolve_bench", "workload": cfg.name, "width": cfg.width, "height": cfg.height,
          "sources_sha": N.build_info()["sources_sha"], "device": torch.cuda.get_device_name(0),
          "bytes_per_pixel": BYTES_READ + BYTES_WRITTEN, "algorithmic_bytes": total, "steps": a.steps})
    with ShadingContext(0) as ctx:
        # (b) the host route, timed first (also the reference planes of the equality check)
        host_s = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            planes, _ = S.fill_gbuffer_host(cfg, n_threads=16)
            t1 = time.perf_counter()
            gb_host = GBuffer.from_host(planes, dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host_s.append((t2 - t0, t1 - t0, t2 - t1))
        host_s.sort()
        b_ms = host_s[len(host_s) // 2][0] * 1e3
        emit({"leg": "b_host_fill_plus_upload", "median_ms": b_ms, "fill_ms": host_s[len(host_s) // 2][1] * 1e3,
              "upload_ms": host_s[len(host_s) // 2][2] * 1e3, "reps": a.host_reps,
              "uploaded_bytes": int(planes.nbytes)})
        ctx.set_materials(*S.scene_materials(cfg))
        attrs = S.build_attributes(cfg, dev, n_threads=16)
        res = {}
        for name, filt in (("point", N.PBR_FILTER_POINT), ("linear", N.PBR_FILTER_LINEAR)):
            out = ctx.resolve(attrs, filt)
            torch.cuda.synchronize()
            if filt == N.PBR_FILTER_POINT:  # the same G-buffer as the host route's, bit for bit
                same = torch.equal(out[0].planes.view(torch.int32), gb_host.planes.view(torch.int32))
                emit({"check": "resolved planes == host fill planes", "bit_identical": bool(same)})
                if not same:
                    sys.exit("resolve_bench: the device resolve differs from the host fill")
            r = event_ms(lambda: ctx.resolve(attrs, filt, out=out), a.steps)
            r.update(leg="a_resolve_" + name, gb_per_s=total / (r["median_ms"] * 1e-3) / 1e9)
            res[name] = r
            emit(r)
        # (d) the trilinear resolve and the chain generation
        gen = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.generate_mips()
            gen.append((time.perf_counter() - t0) * 1e3)
        gen.sort()
        mats, texs = S.scene_materials(cfg)
        emit({"leg": "d_generate_mips", "median_ms": gen[len(gen) // 2], "min_ms": gen[0], "max_ms": gen[-1],
              "textures": len(texs), "level0_texels": int(sum(t.shape[0] * t.shape[1] for t in texs))})
        same = torch.equal(ctx.resolve_mip(attrs, -64.0)[0].planes.view(torch.int32),
                           ctx.resolve(attrs, N.PBR_FILTER_LINEAR)[0].planes.view(torch.int32))
        emit({"check": "trilinear at lod 0 == linear planes", "bit_identical": bool(same)})
        if not same:
            sys.exit("resolve_bench: the trilinear resolve at lod 0 differs from the linear filter")
        for name, bias in (("lod0", -64.0), ("bias0", 0.0), ("bias1.5", 1.5)):
            out = ctx.resolve_mip(attrs, bias)
            r = event_ms(lambda: ctx.resolve_mip(attrs, bias, out=out), a.steps)
            r.update(leg="d_resolve_mip_" + name, lod_bias=bias, gb_per_s=total / (r["median_ms"] * 1e-3) / 1e9,
                     over_linear=r["median_ms"] / res["linear"]["median_ms"])
            res["mip_" + name] = r
            emit(r)
        # (e) the anisotropic resolve beside (d)'s legs of the same run, the yardsticks of these legs
        for bias in (0.0, 1.5):
            same = torch.equal(ctx.resolve_aniso(attrs, 1, bias)[0].planes.view(torch.int32),
                               ctx.resolve_mip(attrs, bias)[0].planes.view(torch.int32))
            emit({"check": "anisotropic with max_anisotropy 1 == trilinear planes", "lod_bias": bias,
                  "bit_identical": bool(same)})
            if not same:
                sys.exit("resolve_bench: the anisotropic resolve with one tap differs from the trilinear resolve")
        # the worst case: the scene's attributes under a UV ramp of 10 : 1 texels per pixel (x : y; every texture of the
        # scene has one size), so every sample whose quad partners are valid takes max_anisotropy = 8 taps, at
        # r2 = 100 / 64 plus a bias of 0.5: between levels 0 and 1, two levels of 8 bilinears each
        size = float(texs[0].shape[1])
        assert all(t.shape[0] == size and t.shape[1] == size for t in texs)
        worst_planes = attrs.planes.clone()
        worst_planes[12] = torch.arange(worst_planes.shape[2], device=dev, dtype=torch.float32)[None, :] * (10.0 / size)
        worst_planes[13] = torch.arange(worst_planes.shape[1], device=dev, dtype=torch.float32)[:, None] * (1.0 / size)
        worst = type(attrs)(worst_planes, attrs.material, attrs.width)
        ids = attrs.material[:attrs.height // 2 * 2, :attrs.width // 2 * 2]  # whole quads
        geometry = (ids.int() & 0xFFFF) < len(mats)
        pairs_x = (ids[:, 0::2] == ids[:, 1::2]).repeat_interleave(2, dim=1)
        pairs_y = (ids[0::2] == ids[1::2]).repeat_interleave(2, dim=0)
        full = float((geometry & pairs_x & pairs_y).sum()) / float(geometry.sum())
        for name, m, bias, at, yard, taps in (("m1_bias0", 1, 0.0, attrs, "mip_bias0", None),
                                             ("m1_bias1.5", 1, 1.5, attrs, "mip_bias1.5", None),
                                             ("m8_bias0", 8, 0.0, attrs, "mip_bias0", None),
                                             ("m8_worst", 8, 0.5, worst, "mip_bias1.5", 16)):
            out = ctx.resolve_aniso(at, m, bias)
            r = event_ms(lambda: ctx.resolve_aniso(at, m, bias, out=out), a.steps)
            y = res[yard]
            r.update(leg="e_resolve_aniso_" + name, max_anisotropy=m, lod_bias=bias,
                     gb_per_s=total / (r["median_ms"] * 1e-3) / 1e9, yardstick="d_resolve_" + yard,
                     over_yardstick=r["median_ms"] / y["median_ms"],
                     yardstick_spread=[y["min_ms"] / y["median_ms"], y["max_ms"] / y["median_ms"]])
            if taps:  # bilinears per sample here against the yardstick's two
                r.update(bilinears_per_sample=taps, samples_with_every_tap=full,
                         ms_per_bilinear_over_yardstick=(r["median_ms"] / taps) / (y["median_ms"] / 2.0))
            emit(r)
        # (c) device-to-device copy moving the same bytes (half read, half written)
        src = torch.empty(total // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        c = event_ms(lambda: dst.copy_(src), a.steps)
        c.update(leg="c_d2d_copy", gb_per_s=total / (c["median_ms"] * 1e-3) / 1e9)
        emit(c)
        emit({"ratios": {"a_point_over_c": res["point"]["median_ms"] / c["median_ms"],
                         "a_linear_over_c": res["linear"]["median_ms"] / c["median_ms"],
                         "b_over_a_point": b_ms / res["point"]["median_ms"],
                         "b_over_a_linear": b_ms / res["linear"]["median_ms"]}})
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
