"""Inputs of tests/test_gpu_resolve_aniso.py beyond those of tests/resolve_mip_cases.py (the material table, the chain
textures, the ramp and special-UV attribute builders): a frame whose every 2 x 2 quad has its own footprint, and the
device call. A helper, not a test. Run as a script (under whatever library PBR_LIB_PATH names -- the bounds-checked
build, in a fresh child process) it writes the device results and the bounds flags to the .npz given."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resolve_cases as C  # noqa: E402
import resolve_mip_cases as MC  # noqa: E402
from physically_based_renderer_amd import _native as N  # noqa: E402

F = np.float32


def quad_attributes(h, w, seed, texels=64):
    """Every 2 x 2 quad its own base UV and its own derivatives: one axis between 1/4 and 2 texels of a square
    `texels`-wide map per pixel, the other longer by a factor between T - 0.95 and T - 0.05, where T walks 1 .. 18 from
    quad to quad (so on that map every tap count 1 .. 16 and the cap sit side by side in any 18 quads of a row of
    quads: in one wave); T = 1 is an exactly isotropic axis-aligned quad, the only footprint with one tap. Either axis
    is the longer one and both have u and v parts. u(x, y) = base + (x & 1) dx + (y & 1) dy, each product and sum
    rounded to float32."""
    rng = np.random.default_rng(seed)
    a = MC.base_attributes(h, w, seed)
    qh, qw = (h + 1) // 2, (w + 1) // 2
    qy, qx = np.meshgrid(np.arange(qh), np.arange(qw), indexing="ij")
    target = (qx * 7 + qy * 5) % 18 + 1  # 7 and 18 are coprime: 18 consecutive quads of a row take 18 values
    short = rng.uniform(0.25, 2.0, (qh, qw))
    long = short * (target - rng.uniform(0.05, 0.95, (qh, qw)))
    ymajor = rng.uniform(size=(qh, qw)) < 0.5
    angle = rng.uniform(0.0, 2.0 * np.pi, (2, qh, qw))
    lx, ly = np.where(ymajor, short, long) / texels, np.where(ymajor, long, short) / texels
    per_quad = [rng.uniform(-1.0, 2.0, (qh, qw)), rng.uniform(-1.0, 2.0, (qh, qw)),   # base u, v
                lx * np.cos(angle[0]), lx * np.sin(angle[0]),                           # dudx, dvdx
                ly * np.cos(angle[1]), ly * np.sin(angle[1])]                           # dudy, dvdy
    # T = 1: dudx = dvdy = a multiple of a quarter texel, dvdx = dudy = 0, the base a multiple of 2^-10: the sums below
    # and the differences the resolve takes are exact, so both footprint lengths are the same float
    iso = target == 1
    step = np.rint(short * 4.0) / 4.0 / texels
    for k in (0, 1):
        per_quad[k][iso] = np.rint(per_quad[k][iso] * 1024.0) / 1024.0
    per_quad[2][iso], per_quad[5][iso] = step[iso], step[iso]
    per_quad[3][iso], per_quad[4][iso] = 0.0, 0.0
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    bu, bv, dudx, dvdx, dudy, dvdy = [p.astype(F)[ys // 2, xs // 2] for p in per_quad]
    fx, fy = (xs & 1).astype(F), (ys & 1).astype(F)
    a[12] = (bu + fx * dudx) + fy * dudy
    a[13] = (bv + fx * dvdx) + fy * dvdy
    return a


def quad_ids(h, w, materials, seed):
    """One of `materials` per 2 x 2 quad, at random: partners stay valid, and no wave has one material."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(materials), ((h + 1) // 2, (w + 1) // 2))
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.asarray(materials, np.uint16)[pick[ys // 2, xs // 2]]


def device_resolve_aniso(ctx, attrs, ids, max_anisotropy, lod_bias=0.0, stride=None, device=None, stream=None,
                         rows=None, pad=False):
    """resolve_cases.device_resolve through ctx.resolve_aniso (``pad``: resolve_cases.padded_inputs)."""
    import torch

    from physically_based_renderer_amd.renderer import Attributes, GBuffer

    device = torch.device("cuda", 0) if device is None else device
    _, h, w = attrs.shape
    stride = w if stride is None else stride
    pa, pi = C.padded_inputs(attrs, ids, stride, pad)
    ta = torch.from_numpy(pa).to(device)
    ti = torch.from_numpy(pi.view(np.int16)).to(device)
    at = Attributes(ta, ti, width=w)
    planes = torch.full((15, h, stride), float(C.SENTINEL), dtype=torch.float32, device=device)
    opacity = torch.full((h, stride), float(C.SENTINEL), dtype=torch.float32, device=device)
    cov = torch.full((h, stride), C.SENTINEL_U8, dtype=torch.uint8, device=device)
    gb = GBuffer(planes, width=w, opacity=opacity)
    torch.cuda.synchronize()
    if rows is None:
        ctx.resolve_aniso(at, max_anisotropy, lod_bias, out=(gb, cov), stream=stream)
    else:
        r0, r1 = rows
        ctx.resolve_aniso(at.rows(r0, r1), max_anisotropy, lod_bias, out=(gb.rows(r0, r1), cov[r0:r1]), stream=stream)
    torch.cuda.synchronize()
    return planes.cpu().numpy(), opacity.cpu().numpy(), cov.cpu().numpy()


TEXTURED = (1, 2, 3, 4, 5, 7, 8, 13, 15)  # of resolve_mip_cases.table(): materials that sample a map


def bounds_cases():
    """The cases the bounds-checked build runs, as (name, attrs, ids, max_anisotropy, lod_bias, stride): the special UVs
    through every material and a frame of per-quad footprints under mixed materials at 70 x 5 (an odd height, an even
    width that is no multiple of the tile's), the scalar and the paired accesses; and both at 71 x 5, an odd width too
    (names with "odd": main() uploads those with a valid-looking padding column)."""
    mats, texs, attrs, ids = MC.bounds_case()
    quads = quad_attributes(5, 70, 77)
    odd_attrs, odd_ids = MC.bounds_case_odd_width()
    return mats, texs, [("special_m8_71", attrs, ids, 8, 0.0, 71), ("special_m16_70", attrs, ids, 16, 1.5, 70),
                        ("quads_m16_70", quads, quad_ids(5, 70, TEXTURED, 78), 16, 0.25, 70),
                        ("quads_m8_71", quads, np.full((5, 70), 7, np.uint16), 8, 0.0, 71),
                        ("odd_special_m8_72", odd_attrs, odd_ids, 8, 0.0, 72),
                        ("odd_quads_m16_71", quad_attributes(5, 71, 79), quad_ids(5, 71, TEXTURED, 80), 16, 0.25, 71)]


def main(out_path):
    """bounds_cases() under the loaded library; the bounds flags of a bounds-checked build."""
    from physically_based_renderer_amd.renderer import ShadingContext

    mats, texs, cases = bounds_cases()
    result = {}
    with ShadingContext(0) as ctx:
        ctx.set_materials(mats, texs)
        ctx.generate_mips()
        for name, attrs, ids, m, bias, stride in cases:
            planes, opacity, cov = device_resolve_aniso(ctx, attrs, ids, m, bias, stride, pad=name.startswith("odd"))
            result[name + "__planes"], result[name + "__opacity"], result[name + "__coverage"] = planes, opacity, cov
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("resolve_aniso under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
