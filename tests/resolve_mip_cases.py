"""Inputs of tests/test_gpu_resolve_mip.py and tests/test_resolve_mip_host.py: a material table over textures of the
sizes whose chains differ in shape (1x1, 5x3, 64x64, 256x1, 3x7; 1, 3 and 4 channels), attribute frames with UV ramps of
a chosen step, and the device call. A helper, not a test. Run as a script (one case under whatever library PBR_LIB_PATH
names -- the bounds-checked build, in a fresh child process) it writes the device result and the bounds flags to the
.npz given."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resolve_cases as C  # noqa: E402
from physically_based_renderer_amd import _native as N  # noqa: E402
from physically_based_renderer_amd.renderer import Material  # noqa: E402

F = np.float32
SHAPES = {"70x37": (37, 70), "256x64": (64, 256)}

# (name, height, width, channels) of the textures whose chains the tests read back; table() lists them first, in order
CHAIN_TEXTURES = [("1x1", 1, 1, 3), ("5x3", 3, 5, 3), ("64x64", 64, 64, 1), ("256x1", 1, 256, 4), ("3x7", 7, 3, 1)]


def table():
    """(materials, textures). Materials 0-8 are resolve_cases.table()'s flag combinations over these textures (7: every
    flag, every map another size; 8: gray maps read as .rgb); 9 + 2 t and 10 + 2 t are two identical diffuse-only
    materials over chain texture t: alternated pixel by pixel they make every partner invalid, so lod = lod_bias."""
    rng = np.random.default_rng(0x31B5)
    tex = lambda h, w, c: rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)
    textures = [tex(h, w, c) for _, h, w, c in CHAIN_TEXTURES]  # 0-4
    textures += [tex(64, 64, 4),   # 5
                 tex(3, 5, 1),     # 6
                 tex(32, 16, 3),   # 7: 16 wide, 32 high
                 tex(128, 128, 1)]  # 8
    const = dict(diffuse_albedo=(0.8, 0.25, 0.1), metallic=0.3, fresnel_r0=(0.04, 0.05, 0.06), roughness=0.45,
                 opacity=0.6)
    D, S_, M, R_, NM, AT = C.D, C.S_, C.M, C.R_, C.NM, C.AT
    materials = [
        Material(**const),                                                           # 0: no flag
        Material(**const, flags=D, tex=(5, -1, -1, -1, -1, -1)),                     # 1: diffuse alone (4 channels)
        Material(**const, flags=S_, tex=(-1, 1, -1, -1, -1, -1)),                    # 2: specular alone (5x3)
        Material(**const, flags=M, tex=(-1, -1, 2, -1, -1, -1)),                     # 3: metallic alone
        Material(**const, flags=R_, tex=(-1, -1, -1, 6, -1, -1)),                    # 4: roughness alone (5x3 gray)
        Material(**const, flags=NM, tex=(-1, -1, -1, -1, 7, -1)),                    # 5: normal alone (16x32)
        Material(**const, flags=AT, tex=(-1, -1, -1, -1, -1, 8)),                    # 6: ALPHA_TEST alone
        Material(**const, flags=D | S_ | M | R_ | NM | AT, tex=(5, 7, 8, 2, 3, 4)),  # 7: every flag, every map a size
        Material(**const, flags=D | NM | AT, tex=(2, -1, -1, -1, 0, 5)),             # 8: gray maps as .rgb, 1x1 normal
    ]
    for t in range(len(CHAIN_TEXTURES)):
        materials += [Material(**const, flags=D, tex=(t, -1, -1, -1, -1, -1))] * 2
    return materials, textures


def base_attributes(h, w, seed):
    """(14, h, w) float32 with ordinary positions, normals and tangent frames; the UV planes are left to the caller."""
    rng = np.random.default_rng(seed)
    a = np.empty((14, h, w), F)
    a[0:3] = rng.uniform(-10, 10, (3, h, w))
    a[3:12] = rng.normal(size=(9, h, w))
    a[12:14] = 0.0
    return a


def ramp_attributes(h, w, du, dv, seed=3, u0=0.0, v0=0.0):
    """UV ramps: u = u0 + x * du, v = v0 + y * dv, each product and sum rounded to float32 (exact for the power-of-two
    steps the tests use)."""
    a = base_attributes(h, w, seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    a[12] = F(u0) + xs * F(du)
    a[13] = F(v0) + ys * F(dv)
    return a


def texel_centre_attributes(h, w, lw, lh, seed=4):
    """Pixel p (row-major) sits on the centre of texel (p % lw, (p // lw) % lh) of a lw x lh level: with lw * lh <=
    h * w every texel of the level lands under some pixel."""
    assert lw * lh <= h * w
    a = base_attributes(h, w, seed)
    p = np.arange(h * w).reshape(h, w)
    a[12] = ((p % lw).astype(F) + F(0.5)) / F(lw)
    a[13] = (((p // lw) % lh).astype(F) + F(0.5)) / F(lh)
    return a


def special_attributes(h, w, n_materials, seed):
    """resolve_cases.attributes with the rows its special UV pairs fill given one material per 2 x 2 quad: there the
    partners are valid, so the footprints are differences of NaN, +-inf, 3e9 and texel-edge coordinates. Below them the
    random pixels, with the background ids, stay as they are."""
    attrs, ids = C.attributes(h, w, n_materials, seed)
    rows = min(len(C.special_uvs()) * n_materials, (h * w * 3) // 5) // w
    ys, xs = np.meshgrid(np.arange(rows), np.arange(w), indexing="ij")
    ids[:rows] = ((xs // 2 + (ys // 2) * ((w + 1) // 2)) % n_materials).astype(np.uint16)
    return attrs, ids


def alternate_ids(h, w, m0, m1):
    """m0 and m1 alternating like a chessboard: every horizontal and vertical partner has the other id."""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.where((xs + ys) % 2 == 0, m0, m1).astype(np.uint16)


def device_resolve_mip(ctx, attrs, ids, lod_bias, stride=None, device=None, stream=None, rows=None, pad=False):
    """resolve_cases.device_resolve through ctx.resolve_mip (``pad``: resolve_cases.padded_inputs)."""
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
        ctx.resolve_mip(at, lod_bias, out=(gb, cov), stream=stream)
    else:
        r0, r1 = rows
        ctx.resolve_mip(at.rows(r0, r1), lod_bias, out=(gb.rows(r0, r1), cov[r0:r1]), stream=stream)
    torch.cuda.synchronize()
    return planes.cpu().numpy(), opacity.cpu().numpy(), cov.cpu().numpy()


def bounds_case():
    """The case the bounds-checked build runs: the special UVs through every material at 70 x 5: an odd height, an even
    width that is no multiple of the tile's."""
    mats, texs = table()
    attrs, ids = special_attributes(5, 70, len(mats), 75)
    return mats, texs, attrs, ids


def bounds_case_odd_width():
    """(attrs, ids) of the same case at 71 x 5: an odd width too, so the last column has no x partner and, in the even
    stride, is the first half of a pair whose second half is padding."""
    return special_attributes(5, 71, len(table()[0]), 76)


# (name, odd width, lod_bias, stride) of the runs of main(); the odd-width ones upload a valid-looking padding column
BOUNDS_RUNS = (("bias0_71", False, 0.0, 71), ("bias1.5_70", False, 1.5, 70),
               ("odd_bias0_71", True, 0.0, 71), ("odd_bias1.5_72", True, 1.5, 72))


def main(out_path):
    """bounds_case() and bounds_case_odd_width() under the loaded library, scalar and paired accesses; the bounds flags of
    a bounds-checked build."""
    from physically_based_renderer_amd.renderer import ShadingContext

    mats, texs, attrs, ids = bounds_case()
    odd = bounds_case_odd_width()
    result = {}
    with ShadingContext(0) as ctx:
        ctx.set_materials(mats, texs)
        ctx.generate_mips()
        for name, odd_width, bias, stride in BOUNDS_RUNS:
            a, i = odd if odd_width else (attrs, ids)
            planes, opacity, cov = device_resolve_mip(ctx, a, i, bias, stride, pad=odd_width)
            result[name + "__planes"], result[name + "__opacity"], result[name + "__coverage"] = planes, opacity, cov
        flagged = ctx.debug_bounds()
        result["bounds"] = np.array([flagged.get(k, -1) for k in ("gbuffer", "output", "coverage", "texel", "light",
                                                                  "lds")], np.int64)
    unit = next(u for u in N.build_info()["units"] if u["unit"] == "frontend_kernels")
    result["flavor"], result["sources_sha"] = np.array(unit["flavor"]), np.array(unit["sources_sha"])
    np.savez(out_path, **result)
    print("resolve_mip under", N.LIB_PATH, "bounds", flagged)


if __name__ == "__main__":
    main(sys.argv[1])
