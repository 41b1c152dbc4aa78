"""Inputs of tests/test_gpu_resolve.py: a material table with one material per flag combination that matters,
textures of every size class and channel count, and attribute frames whose UVs walk every special value through every
material. A helper, not a test. Run as a script (one case under whatever library PBR_LIB_PATH names -- the
bounds-checked build, in a fresh child process, as tests/bounds_cases.py does) it writes the device result and the
bounds flags to the .npz given."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from physically_based_renderer_amd import _native as N  # noqa: E402
from physically_based_renderer_amd.renderer import Material  # noqa: E402

DEBUG_LIB = os.path.join(ROOT, "physically_based_renderer_amd", "_lib", "debug_bounds", "libpbrshade.so")
SENTINEL = np.float32(-12345.25)
SENTINEL_U8 = 0xA5

D, S_, M, R_, NM, AT = (N.PBR_MAT_DIFFUSE_TEXTURE, N.PBR_MAT_SPECULAR_TEXTURE, N.PBR_MAT_METALLIC_TEXTURE,
                        N.PBR_MAT_ROUGHNESS_TEXTURE, N.PBR_MAT_NORMAL_TEXTURE, N.PBR_MAT_ALPHA_TEST)


def table():
    """(materials, textures): 1x1, 5x3, 64x64 and 256x256 textures with 1, 3 and 4 channels; each texture flag alone,
    all flags, none, ALPHA_TEST with and without others."""
    rng = np.random.default_rng(0x7AB1E)
    tex = lambda h, w, c: rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)
    textures = [tex(1, 1, 3),       # 0
                tex(3, 5, 3),       # 1: 5 wide, 3 high
                tex(64, 64, 1),     # 2
                tex(256, 256, 4),   # 3
                tex(3, 5, 1),       # 4
                tex(64, 64, 3),     # 5
                tex(1, 1, 1),       # 6
                tex(256, 256, 1),   # 7
                tex(64, 64, 4)]     # 8
    const = dict(diffuse_albedo=(0.8, 0.25, 0.1), metallic=0.3, fresnel_r0=(0.04, 0.05, 0.06), roughness=0.45,
                 opacity=0.6)
    materials = [
        Material(**const),                                                        # 0: no flag
        Material(**const, flags=D, tex=(3, -1, -1, -1, -1, -1)),                  # 1: diffuse alone (4 channels)
        Material(**const, flags=S_, tex=(-1, 1, -1, -1, -1, -1)),                 # 2: specular alone (5x3)
        Material(**const, flags=M, tex=(-1, -1, 2, -1, -1, -1)),                  # 3: metallic alone
        Material(**const, flags=R_, tex=(-1, -1, -1, 4, -1, -1)),                 # 4: roughness alone (5x3 gray)
        Material(**const, flags=NM, tex=(-1, -1, -1, -1, 5, -1)),                 # 5: normal alone
        Material(**const, flags=AT, tex=(-1, -1, -1, -1, -1, 7)),                 # 6: ALPHA_TEST alone
        Material(**const, flags=D | S_ | M | R_ | NM | AT, tex=(8, 0, 6, 2, 1, 4)),  # 7: every flag, mixed sizes
        Material(**const, flags=D | NM | AT, tex=(2, -1, -1, -1, 6, 3)),          # 8: gray maps read as .rgb, 4-ch opacity
    ]
    return materials, textures


def special_uvs():
    """(u, v) pairs: negatives, > 1, exactly 0 and 1, texel edges k / W of every texture width and height, NaN, +-inf
    and 3e9 (beyond wrap_index's 2e9 guard)."""
    f = np.float32
    edges = [f(k) / f(n) for n in (3, 5, 64, 256) for k in (1, 2, n - 1, n, n + 1, -1)]
    vals = [f(0.0), f(-0.0), f(1.0), f(-0.25), f(-1.0), f(-7.3), f(1.5), f(2.0), f(123.456), f(np.nan), f(np.inf),
            f(-np.inf), f(3.0e9), f(-3.0e9), f(1.9e9), f(0.999999)] + edges
    pairs = [(u, vals[(i * 7 + 3) % len(vals)]) for i, u in enumerate(vals)]
    pairs += [(f(0.5), f(np.nan)), (f(np.inf), f(0.25)), (f(0.0), f(0.0)), (f(1.0), f(1.0))]
    return pairs


def attributes(h, w, n_materials, seed):
    """(attrs (14, h, w) float32, ids (h, w) uint16): the special UV pairs cycled through the materials over (at most)
    the first 60% of the pixels, then random pixels with background ids 0xFFFF and n_materials + 1 sprinkled in; one
    zero-length NormalW."""
    rng = np.random.default_rng(seed)
    a = np.empty((14, h, w), np.float32)
    a[0:3] = rng.uniform(-10, 10, (3, h, w))
    a[3:12] = rng.normal(size=(9, h, w))
    a[12:14] = rng.uniform(-2.0, 3.0, (2, h, w))
    ids = rng.integers(0, n_materials, (h, w)).astype(np.uint16)
    bg = rng.uniform(size=(h, w))
    ids[bg < 0.06] = N.PBR_MATERIAL_NONE
    ids[(bg >= 0.06) & (bg < 0.12)] = n_materials + 1
    flat_u, flat_v, flat_i = a[12].reshape(-1), a[13].reshape(-1), ids.reshape(-1)
    pairs = special_uvs()  # 44 pairs, coprime with the 9 materials: pixel k takes pair k under material k
    for k in range(min(len(pairs) * n_materials, (h * w * 3) // 5)):
        flat_u[k], flat_v[k] = pairs[k % len(pairs)]
        flat_i[k] = k % n_materials
    # textured material, ordinary UV, zero-length normal: normalize gives NaN (Default.hlsl:50)
    zy, zx = h - 1, w // 2
    a[3:6, zy, zx] = 0.0
    ids[zy, zx] = 5
    a[12:14, zy, zx] = 0.3
    return a, ids


def uniform_ids(h, w, n_materials):
    """Every wave (64 x 2 pixels) one material, a few background pixels inside (they do not break uniformity)."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ids = (((xs // 64) + (ys // 2) * ((w + 63) // 64)) % n_materials).astype(np.uint16)
    ids[(xs * 7 + ys * 3) % 23 == 0] = N.PBR_MATERIAL_NONE
    return ids


def checker_ids(h, w, n_materials):
    """Materials alternate pixel by pixel: both pixels of every lane differ, no wave is uniform."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((xs + ys * 4) % n_materials).astype(np.uint16)


def padded_inputs(attrs, ids, stride, pad=False):
    """(attrs (14, h, stride) float32, ids (h, stride) uint16) as the device helpers upload them. Default: the padding
    columns hold NaN and id 0xFFFF. ``pad``: they hold a believable geometry pixel instead -- the id of the row's last
    column, its attributes where they are finite (0.5 where not), and UVs that continue the row's ramp (the last
    column plus one, two ... times the step between the last two columns; 1 / 8 where the row has one column or the
    step is not finite) -- so a kernel that took a padding column for a partner would see a valid one."""
    _, h, w = attrs.shape
    a = np.full((14, h, stride), np.nan, np.float32)
    i = np.full((h, stride), 0xFFFF, np.uint16)
    a[:, :, :w], i[:, :w] = attrs, ids
    if pad and stride > w:
        with np.errstate(all="ignore"):
            last = np.where(np.isfinite(attrs[:, :, w - 1]), attrs[:, :, w - 1], np.float32(0.5))
            step = attrs[12:14, :, w - 1] - attrs[12:14, :, w - 2] if w >= 2 else np.full((2, h), np.nan, np.float32)
            step = np.where(np.isfinite(step), step, np.float32(0.125)).astype(np.float32)
            for j in range(stride - w):
                a[:, :, w + j] = last
                a[12:14, :, w + j] = last[12:14] + np.float32(j + 1) * step
                i[:, w + j] = ids[:, w - 1]
    return a, i


def device_resolve(ctx, attrs, ids, filt, stride=None, device=None, stream=None, rows=None, pad=False):
    """Upload (with `stride` elements per row), resolve into sentinel-filled canvases of the same stride, return
    (planes (15, h, stride), opacity (h, stride), coverage (h, stride)) as numpy, synchronised. ``pad``: the input
    padding columns hold a valid-looking pixel (padded_inputs) instead of NaN and id 0xFFFF."""
    import torch

    from physically_based_renderer_amd.renderer import Attributes, GBuffer

    device = torch.device("cuda", 0) if device is None else device
    _, h, w = attrs.shape
    stride = w if stride is None else stride
    pa, pi = padded_inputs(attrs, ids, stride, pad)
    ta = torch.from_numpy(pa).to(device)
    ti = torch.from_numpy(pi.view(np.int16)).to(device)
    at = Attributes(ta, ti, width=w)
    planes = torch.full((15, h, stride), float(SENTINEL), dtype=torch.float32, device=device)
    opacity = torch.full((h, stride), float(SENTINEL), dtype=torch.float32, device=device)
    cov = torch.full((h, stride), SENTINEL_U8, dtype=torch.uint8, device=device)
    gb = GBuffer(planes, width=w, opacity=opacity)
    torch.cuda.synchronize()
    if rows is None:
        ctx.resolve(at, filt, out=(gb, cov), stream=stream)
    else:
        r0, r1 = rows
        ctx.resolve(at.rows(r0, r1), filt, out=(gb.rows(r0, r1), cov[r0:r1]), stream=stream)
    torch.cuda.synchronize()
    return planes.cpu().numpy(), opacity.cpu().numpy(), cov.cpu().numpy()


def main(out_path):
    """One case of the random-attribute test under the loaded library; the bounds flags of a bounds-checked build."""
    from physically_based_renderer_amd.renderer import ShadingContext

    mats, texs = table()
    attrs, ids = attributes(3, 70, len(mats), 70)
    result = {}
    with ShadingContext(0) as ctx:
        ctx.set_materials(mats, texs)
        for name, filt, stride in (("point_71", N.PBR_FILTER_POINT, 71), ("linear_70", N.PBR_FILTER_LINEAR, 70)):
            planes, opacity, cov = device_resolve(ctx, attrs, ids, filt, stride)
            result[name + "__planes"], result[name + "__opacity"], result[name + "__coverage"] = planes, opacity, cov
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")  # the resolve kernel's unit
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("resolve under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
