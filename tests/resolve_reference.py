"""The material resolve (pbr_resolve_materials; Default.hlsl:50-116) restated in numpy fp32, one numpy
operation per HLSL operation: every intermediate is a float32 array, so each +, -, *, / and sqrt rounds once, as the
canonical fp32 semantics of DESIGN.md §2 ask (no contraction, correctly rounded / and sqrt). A helper, not a test:
tests/test_resolve_host.py ties it to the host fill, tests/test_gpu_resolve.py holds the device kernel to it bit for
bit."""
import numpy as np

from physically_based_renderer_amd import _native as N

F = np.float32
POINT, LINEAR = N.PBR_FILTER_POINT, N.PBR_FILTER_LINEAR


def decode_unorm8(u8):
    """(float)u8 / 255.0f."""
    return u8.astype(F) / F(255.0)


def wrap_index(f, n):
    """wrap_index of oracle/pbr_oracle.c:172-176: (int)f % n, plus n when negative; NaN or |f| > 2e9 gives 0."""
    bad = np.isnan(f) | (f > F(2.0e9)) | (f < F(-2.0e9))
    i = np.where(bad, F(0.0), f).astype(np.int64)  # (int)f truncates; f is integral here (a floorf result)
    return np.where(bad, 0, np.mod(i, n))  # floor-mod == C's truncating % plus n when negative


def lerp(a, b, t):
    return a + t * (b - a)


def _texture(t):
    t = np.asarray(t)
    assert t.dtype == np.uint8
    return t if t.ndim == 3 else t[:, :, None]


def _channels(texels_u8, nch):
    """(n, C) taps -> nch decoded channel arrays; a 1-channel texture read as .rgb replicates .r."""
    c_in = texels_u8.shape[1]
    return [decode_unorm8(texels_u8[:, c if c_in > 1 else 0]) for c in range(nch)]


def sample(tex, u, v, filt, nch):
    """nch channels of UNORM8 texture `tex` at float32 (u, v): point-wrap or linear-wrap bilinear."""
    tex = _texture(tex)
    h, w = tex.shape[0], tex.shape[1]
    with np.errstate(all="ignore"):
        if filt == POINT:
            tx = wrap_index(np.floor(u * F(w)), w)
            ty = wrap_index(np.floor(v * F(h)), h)
            return _channels(tex[ty, tx], nch)
        x = u * F(w) - F(0.5)
        y = v * F(h) - F(0.5)
        x0f, y0f = np.floor(x), np.floor(y)
        fx, fy = x - x0f, y - y0f
        x0, y0 = wrap_index(x0f, w), wrap_index(y0f, h)
        x1 = np.where(x0 + 1 == w, 0, x0 + 1)
        y1 = np.where(y0 + 1 == h, 0, y0 + 1)
        t00, t10 = _channels(tex[y0, x0], nch), _channels(tex[y0, x1], nch)
        t01, t11 = _channels(tex[y1, x0], nch), _channels(tex[y1, x1], nch)
        return [lerp(lerp(t00[c], t10[c], fx), lerp(t01[c], t11[c], fx), fy) for c in range(nch)]


def resolve(attrs, material, materials, textures, filt=POINT):
    """attrs (14, H, W) float32 (pos, normal, tangent, bitangent, uv), material (H, W) uint16, `materials` a list of
    renderer.Material, `textures` a list of uint8 arrays -> (planes (15, H, W) float32, opacity (H, W) float32,
    coverage (H, W) uint8)."""
    attrs = np.asarray(attrs, F)
    material = np.asarray(material).astype(np.int64) & 0xFFFF
    hh, ww = material.shape
    planes = np.empty((15, hh, ww), F)
    # background (gbuffer_fill.cpp:264-275): position and NormalW pass through
    planes[0:3] = attrs[0:3]
    planes[3:6] = attrs[3:6]
    planes[6:9] = F(0.0)
    planes[9] = F(0.0)
    planes[10] = F(1.0)
    planes[11] = F(1.0)
    planes[12:15] = F(0.04)
    opacity = np.full((hh, ww), F(1.0), F)
    coverage = np.zeros((hh, ww), np.uint8)
    with np.errstate(all="ignore"):
        for mid, m in enumerate(materials):
            sel = material == mid
            if not sel.any():
                continue
            a = attrs[:, sel]
            nx, ny, nz = a[3], a[4], a[5]
            length = np.sqrt((nx * nx + ny * ny) + nz * nz)  # normalize(pin.NormalW), Default.hlsl:50
            nw = [nx / length, ny / length, nz / length]
            u, v = a[12], a[13]
            fl, tex = int(m.flags), [int(t) for t in m.tex]
            n = u.shape[0]
            const = lambda val: np.full(n, F(val), F)
            if fl & N.PBR_MAT_DIFFUSE_TEXTURE:
                alb = sample(textures[tex[0]], u, v, filt, 3)
            else:
                alb = [const(c) for c in m.diffuse_albedo]
            if fl & N.PBR_MAT_METALLIC_TEXTURE:
                metal = sample(textures[tex[2]], u, v, filt, 1)[0]
            else:
                metal = const(m.metallic)
            if fl & N.PBR_MAT_SPECULAR_TEXTURE:
                f0 = sample(textures[tex[1]], u, v, filt, 3)
            else:
                f0 = [lerp(const(m.fresnel_r0[c]), alb[c], metal) for c in range(3)]  # Default.hlsl:94-95
            if fl & N.PBR_MAT_ROUGHNESS_TEXTURE:
                rough = sample(textures[tex[3]], u, v, filt, 1)[0]
            else:
                rough = const(m.roughness)
            if fl & N.PBR_MAT_NORMAL_TEXTURE:  # NormalSampleToWorldSpace, LightingUtil.hlsl:203-214
                s = sample(textures[tex[4]], u, v, filt, 3)
                nt = [F(2.0) * s[c] - F(1.0) for c in range(3)]
                nrm = [(nt[0] * a[6 + c] + nt[1] * a[9 + c]) + nt[2] * nw[c] for c in range(3)]
            else:
                nrm = nw
            if fl & N.PBR_MAT_ALPHA_TEST:  # always g_SamPointWrap, Default.hlsl:112
                opa = sample(textures[tex[5]], u, v, POINT, 1)[0]
            else:
                opa = const(m.opacity)
            for c in range(3):
                planes[3 + c][sel] = nrm[c]
                planes[6 + c][sel] = alb[c]
                planes[12 + c][sel] = f0[c]
            planes[9][sel] = metal
            planes[10][sel] = rough
            opacity[sel] = opa
            coverage[sel] = 1
    return planes, opacity, coverage
